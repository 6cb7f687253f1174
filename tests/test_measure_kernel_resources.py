"""sx_result_measure_device, what the compiler made of stringsext_amd/csrc/sx_measure_dev.hip (no GPU needed): the per-kernel
resource remarks the Makefile keeps next to the object."""
from test_fold_kernel_resources import constant
from test_kernel_resources import remarks

KERNELS = ["measure_narrow_kernel", "measure_wide_kernel"]


def test_the_measure_kernels_have_no_scratch_no_spills_and_their_counters_fit_a_cu():
    rows = remarks("sx_measure_dev")
    assert sorted(rows) == KERNELS, sorted(rows)
    waves, groups = constant("sx_measure_dev.hip", "kMeasureWaves"), constant("sx_measure_dev.hip", "kMeasureGroupsPerCu")
    wide_groups, rows_waves = constant("sx_measure_dev.hip", "kMeasureWideGroupsPerCu"), constant("sx_rows_dev.hpp", "kRowsWaves")
    table = 256 * 4                                                          # c x LG(c), c < 256
    want = {"measure_narrow_kernel": (table + waves * 64 * 256, groups, waves),                # a byte per lane and value
            "measure_wide_kernel": (table + rows_waves * 256 * 4, wide_groups, rows_waves)}      # a word per wavefront and value
    for k, v in rows.items():
        lds, per_cu, w = want[k]
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0 and v["Dynamic Stack"] == "False", (k, v)
        assert v["LDS Size [bytes/block]"] == lds, (k, v)                # what the source states: no array of a lane's went there
        assert per_cu * v["LDS Size [bytes/block]"] <= 160 * 1024, (k, v)      # a CU of gfx950 has 160 KiB
        # the grid's workgroups per CU are resident together only if the registers allow as many wavefronts, over 4 SIMDs;
        # tests/test_gpu_measure_device.py's second trip rests on the same numbers
        assert v["Occupancy [waves/SIMD]"] * 4 >= per_cu * w, (k, v)
