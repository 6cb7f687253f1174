"""sx_result_order_device, what the compiler made of stringsext_amd/csrc/sx_order_dev.hip (no GPU needed): the per-kernel resource
remarks the Makefile keeps next to the object.  The file also instantiates rocprim's sorts and scans; their kernels are not ours and
are not judged here."""
from test_kernel_resources import remarks

KERNELS = ["order_compact_kernel", "order_field_kernel", "order_gather_kernel", "order_gkey_kernel", "order_measure_kernel", "order_number_kernel",
           "order_pick_kernel", "order_split_kernel", "order_wkey_kernel", "order_word_kernel"]


def test_the_order_kernels_are_there_with_no_scratch_no_spills_no_lds_and_eight_wavefronts_per_simd():
    rows = {k: v for k, v in remarks("sx_order_dev").items() if not k.startswith("rocprim::")}
    assert sorted(rows) == KERNELS, sorted(rows)
    for k, v in rows.items():
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0 and v["Dynamic Stack"] == "False", (k, v)
        assert v["LDS Size [bytes/block]"] == 0, (k, v)
        # the grid: kOrderGroupsPerCu = 4 workgroups of 8 wavefronts per CU are 8 wavefronts per SIMD, and all of them are resident
        # only if the registers allow 8 — the stride of tests/test_gpu_order_device.py's strided trip rests on the same numbers
        assert v["Occupancy [waves/SIMD]"] >= 8, (k, v)
