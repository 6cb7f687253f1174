"""sx_result_fuzzy_device, what the compiler made of stringsext_amd/csrc/sx_fuzzy_dev.hip (no GPU needed): the per-kernel resource
remarks the Makefile keeps next to the object.  The kernel's layout rests on its registers — a group of patterns is what a lane holds
at once —, so a spill or scratch would be a slow kernel that still passes every other test."""
from test_kernel_resources import remarks


def test_both_fuzzy_kernels_are_there_with_no_spills_and_no_scratch_and_three_workgroups_fit_a_cu():
    rows = remarks("sx_fuzzy_dev")
    assert sorted(rows) == ["fuzzy_match_kernel<unsigned int>", "fuzzy_match_kernel<unsigned long>"], sorted(rows)
    for k, v in rows.items():
        assert v["VGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        lds = v["LDS Size [bytes/block]"]
        assert lds == 512 + 48 * 1024 + 64 * 4 + 64 * 8, lds                    # the class map, the rows, the counters, the minima
        assert 3 * lds <= 160 * 1024                                              # kRowsGroupsPerCu; a CU of gfx950 has 160 KiB
        assert v["Occupancy [waves/SIMD]"] >= 6, (k, v)                           # three workgroups of eight wavefronts on four SIMDs
