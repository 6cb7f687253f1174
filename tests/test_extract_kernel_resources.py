"""sx_result_extract_regex_device, what the compiler made of stringsext_amd/csrc/sx_extract_dev.hip (no GPU needed): the per-kernel
resource remarks the Makefile keeps next to the object."""
from test_kernel_resources import remarks


def test_the_two_extract_kernels_are_there_with_no_scratch_and_no_spills_and_three_workgroups_fit_a_cu():
    rows = remarks("sx_extract_dev")
    ours = sorted(k for k in rows if k.startswith("extract_"))
    assert ours == ["extract_count_kernel", "extract_place_kernel"], sorted(rows)
    for k, v in rows.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
    for k in ours:
        assert 3 * rows[k]["LDS Size [bytes/block]"] <= 160 * 1024, rows[k]      # kExtractGroupsPerCu; a CU of gfx950 has 160 KiB
