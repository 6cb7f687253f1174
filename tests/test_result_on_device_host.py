"""SX_OPT_RESULT_ON_DEVICE with several Missions, the parts that need no GPU: the gather kernel's resources as the compiler
reports them, and the fallback of a host-only context (include/stringsext_amd.h: its result stays in host memory)."""
import random

import refconfig as rc
import stringsext_amd as sx
import sxo_binding as sxo
from product_harness import oracle_runs_for_chunk
from test_host_logic import synth
from test_kernel_resources import remarks


def test_the_gather_kernel_has_no_scratch_and_no_spills():
    rows = remarks("sx_result_dev")
    assert "result_gather_kernel" in rows, sorted(rows)
    v = rows["result_gather_kernel"]
    assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, v


def test_a_host_only_context_with_two_missions_keeps_a_host_result():
    rng = random.Random(2026)
    data = synth(rng, 600_000, 1 / 300)
    ms = rc.missions(encodings=["utf-8", "utf-16le"], chars_min="10")
    want = sxo.run_cli(ms, [data], radix="x")
    assert b"(a " in want and b"(b " in want
    sc = sx.Scanner(ms, device=sx.SX_HOST_ONLY, result_on_device=True)
    try:
        res = sc.replay_runs(data, oracle_runs_for_chunk(ms, data, 0), file_id=1)
        segs = res.device_segments()
        assert segs and all(s[0] is None for s in segs)
        assert sx.OUTPUT_BOM + res.printed(n_inputs=1, radix="x") + b"\n" == want
        res.free()
    finally:
        sc.close()
