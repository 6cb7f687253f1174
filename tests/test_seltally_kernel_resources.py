"""sx_result_tally_device, what the compiler made of stringsext_amd/csrc/sx_seltally_dev.hip (no GPU needed): the per-kernel resource
remarks the Makefile keeps next to the object."""
from test_kernel_resources import remarks


def test_the_tally_kernel_is_there_twice_with_no_scratch_and_no_spills_and_two_workgroups_fit_a_cu():
    rows = remarks("sx_seltally_dev")
    assert sorted(rows) == ["seltally_kernel<unsigned int>", "seltally_kernel<unsigned short>"], sorted(rows)   # 4- and 2-byte entries, nothing else
    for k, v in rows.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert 2 * v["LDS Size [bytes/block]"] <= 160 * 1024, v      # a CU of gfx950 has 160 KiB of LDS
