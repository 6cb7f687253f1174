"""sx_result_select_regex_device, what the compiler made of stringsext_amd/csrc/sx_selre_dev.hip (no GPU needed): the per-kernel
resource remarks the Makefile keeps next to the object."""
from test_kernel_resources import remarks


def test_the_regex_kernel_is_there_with_no_scratch_and_no_spills_and_three_workgroups_fit_a_cu():
    rows = remarks("sx_selre_dev")
    ours = sorted(k for k in rows if k.startswith("selre_match_kernel"))
    assert ours == ["selre_match_kernel"], sorted(rows)
    assert not any(k.startswith("select_") or k.startswith("selset_") for k in rows)
    for k, v in rows.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
    assert 3 * rows["selre_match_kernel"]["LDS Size [bytes/block]"] <= 160 * 1024, rows["selre_match_kernel"]   # kSelreGroupsPerCu; a CU of gfx950 has 160 KiB
