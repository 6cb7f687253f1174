"""What the compiler made of the device formatter's kernels (stringsext_amd/csrc/sx_print_dev.hip; no GPU needed): none of them —
the length pass, the write pass, the scan between them — has vector-register spill code or a stack.  These are conditions, not
measurements: a formatter that keeps the position's digits in an indexed per-lane array gets that array in scratch memory."""
from test_kernel_resources import remarks


def test_print_kernels_have_no_spills_and_no_scratch():
    rows = remarks("sx_print_dev")
    own = {k: v for k, v in rows.items() if k.startswith("print_")}
    assert sorted(own) == ["print_len_kernel", "print_write_kernel"], sorted(rows)
    for k, v in rows.items():
        assert v["VGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
