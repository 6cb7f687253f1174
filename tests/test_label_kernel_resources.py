"""sx_result_label_device and sx_result_select_labels_device, what the compiler made of stringsext_amd/csrc/sx_label_dev.hip (no GPU
needed): the per-kernel resource remarks the Makefile keeps next to the object."""
from test_kernel_resources import remarks


def test_the_two_label_kernels_are_there_with_no_scratch_and_no_spills_and_three_workgroups_fit_a_cu():
    rows = remarks("sx_label_dev")
    assert sorted(rows) == ["label_match_kernel", "label_pick_kernel"], sorted(rows)
    for k, v in rows.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
    lds = rows["label_match_kernel"]["LDS Size [bytes/block]"]
    assert lds == 256 + 48 * 1024 + 64 * 4 + 64 * 8, lds                     # the class map, the rows, the counters, the minima
    assert 3 * lds <= 160 * 1024                                                # kLabelGroupsPerCu; a CU of gfx950 has 160 KiB
    assert rows["label_pick_kernel"]["LDS Size [bytes/block]"] == 0
