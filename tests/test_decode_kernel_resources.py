"""sx_result_decode_device, what the compiler made of stringsext_amd/csrc/sx_decode_dev.hip (no GPU needed): the per-kernel resource
remarks the Makefile keeps next to the object.  The file also instantiates rocprim's scan; its kernels are not ours and are not
judged here."""
from test_fold_kernel_resources import constant
from test_kernel_resources import remarks

KERNELS = ["decode_measure_kernel", "decode_place_kernel"]


def test_the_decode_kernels_have_no_scratch_no_spills_no_lds_and_three_workgroups_per_cu():
    rows = {k: v for k, v in remarks("sx_decode_dev").items() if not k.startswith("rocprim::")}
    assert sorted(rows) == KERNELS, sorted(rows)
    groups, waves = constant("sx_rows_dev.hpp", "kRowsGroupsPerCu"), constant("sx_rows_dev.hpp", "kRowsWaves")
    for k, v in rows.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0 and v["Dynamic Stack"] == "False", (k, v)
        assert v["LDS Size [bytes/block]"] == 0, (k, v)                   # the decoder has no table, and no array of a lane's went there
        # the grid: kRowsGroupsPerCu workgroups of kRowsWaves wavefronts per CU, over 4 SIMDs — resident together only if the
        # registers allow as many; R of tests/test_gpu_decode_device.py rests on the same numbers
        assert v["Occupancy [waves/SIMD]"] * 4 >= groups * waves, (k, v)
