"""sx_result_select_device, what the compiler made of stringsext_amd/csrc/sx_select_dev.hip (no GPU needed): the per-kernel
resource remarks the Makefile keeps next to the object."""
from test_kernel_resources import remarks


def test_the_select_kernels_have_no_scratch_and_no_spills():
    rows = remarks("sx_select_dev")
    ours = sorted(k for k in rows if k.startswith("select_"))
    assert ours == ["select_match_kernel", "select_place_kernel"], sorted(rows)
    for k, v in rows.items():   # (the scans' kernels are rows of this object too)
        assert v["VGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
