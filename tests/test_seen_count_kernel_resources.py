"""A seen set that counts, what the compiler made of stringsext_amd/csrc/sx_seen_count_dev.hip (no GPU needed): the per-kernel resource
remarks the Makefile keeps next to the object."""
from test_kernel_resources import remarks


def test_the_four_count_kernels_are_there_with_no_scratch_no_spills_and_no_lds():
    rows = remarks("sx_seen_count_dev")
    assert sorted(rows) == ["label_range_pick_kernel", "seen_count_kernel", "seen_counts_lookup_kernel", "seen_merge_count_kernel"], sorted(rows)
    for k, v in rows.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["LDS Size [bytes/block]"] == 0, (k, v)                          # kSeenCountGroupsPerCu rests on it
        assert v["Occupancy [waves/SIMD]"] >= 8, (k, v)                          # 8 x 4 SIMDs: the 32 wavefronts per CU of the grid
