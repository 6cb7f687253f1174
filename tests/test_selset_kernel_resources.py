"""sx_result_select_set_device, what the compiler made of stringsext_amd/csrc/sx_selset_dev.hip (no GPU needed): the per-kernel
resource remarks the Makefile keeps next to the object."""
from test_kernel_resources import remarks


def test_the_set_kernel_is_there_with_no_scratch_and_no_spills_and_two_workgroups_fit_a_cu():
    rows = remarks("sx_selset_dev")
    ours = sorted(k for k in rows if k.startswith("selset_match_kernel"))
    assert ours == ["selset_match_kernel<unsigned int>", "selset_match_kernel<unsigned short>"], sorted(rows)   # 4- and 2-byte entries
    assert not any(k.startswith("select_") for k in rows)
    for k, v in rows.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
    for k in ours:
        assert 2 * rows[k]["LDS Size [bytes/block]"] <= 160 * 1024, rows[k]      # a CU of gfx950 has 160 KiB of LDS
