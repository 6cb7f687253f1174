"""What the strings of a device-resident result look like (sx_result_measure_device) against its yardsticks: BASELINE config 5's
Missions on GIB GiB of background, as tools/gpu_fold.py.
usage: tools/gpu_measure.py [--reps N] [--out FILE] [GIB ...]      (default: 4; profiler off)
After a warm-up of every path, alternating, N times each (default 5), the host clock around calls that end synchronised:
  measure     one sx_result_measure_device call: a word per finding, with sx_measure_info
  everything  sx_result_select_device with a pattern that cannot occur, inverted: the whole part selected and gathered —
              result_gather_kernel's time on it is the yardstick of DESIGN.md §7 item 7
  entropy     sx_result_select_labels_range_device on the words: the findings of 4.5 bits per byte and more
  download    the records and the strings of every segment copied to the host (sx_device_download) into pinned memory, as
              tools/gpu_order.py copies them: what a host that measures needs first
Checked once, outside the timed region: the words of the first 200 000 findings of segment 0 are the rule's, restated here in Python
as include/stringsext_amd.h states it, and sx_measure_info's findings and bytes are the segments'.  One JSON line per size (stdout,
and appended to FILE).
Kernel times: run this under `rocprofv3 --kernel-trace --stats` with `--reps 2 4`, a run of its own: per call and segment the launches
are measure_narrow_kernel and measure_wide_kernel."""
import collections
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import stringsext_amd as sx
from gpu_order import PINNED, download as download_pinned
from gpu_select import C5, F16, SEED, stat

CANNOT_OCCUR = b"\x02\x02"


# The rule once more, independent of the library: it must say what include/stringsext_amd.h says (as tests/measure_plant.py does)
def lg16(x):
    e = x.bit_length() - 1
    m, f = x << (31 - e), 0
    for _ in range(16):
        m = (m * m) >> 31
        f <<= 1
        if m >= 1 << 32:
            f |= 1
            m >>= 1
    return e << 16 | f


def byte_class(b):
    for lo, hi, bit in ((0x61, 0x7A, 25), (0x41, 0x5A, 26), (0x30, 0x39, 27), (0x20, 0x20, 28), (0x09, 0x09, 28), (0x21, 0x7E, 29), (0x80, 0xFF, 31)):
        if lo <= b <= hi:
            return 1 << bit
    return 1 << 30


def measure(s):
    n, count = len(s), collections.Counter(s)
    if n == 0:
        return 0
    t = n * lg16(n) - sum(c * lg16(c) for c in count.values())
    word = min(65535, t // (16 * n)) | len(count) << 16 | (n - sum(c for b, c in count.items() if 0x80 <= b <= 0xBF)) << 32
    for b in count:
        word |= byte_class(b)
    return word


def main():
    args, reps, out = sys.argv[1:], 5, None
    while args and args[0].startswith("--"):
        if args[0] == "--reps":
            reps = int(args[1])
        elif args[0] == "--out":
            out = args[1]
        else:
            sys.exit(__doc__)
        args = args[2:]
    ms = sx.missions_from_flags(**C5)
    for gib in [float(a) for a in args] or [4]:
        total = int(gib * (1 << 30)) // 4096 * 4096
        sc = sx.Scanner(ms, device=0, result_on_device=True)
        d = sc.alloc(total)
        sc.fill_background(d, 0, total, SEED)
        sc.reset()
        res = sc.scan_device(d, total, file_id=1)
        segs = res.device_segments()
        assert all(s[0] is not None for s in segs)

        def timed(call):
            t0 = time.perf_counter()
            got = call()
            return (time.perf_counter() - t0) * 1e3, got

        # warm-up of all paths, and the checks
        findings, str_bytes, n_segs = len(res), sum(s[3] for s in segs), len(segs)
        _, m = timed(res.measure_device)
        info = m.info
        assert info["findings"] == findings and info["bytes"] == str_bytes, (info, findings, str_bytes)
        fp, n0, ap, _, packed, _ = segs[0]
        assert packed
        k = min(n0, 200_000)
        recs = np.frombuffer(sc.download(C.c_void_p(fp), k * 16), dtype=F16)
        arena = sc.download(C.c_void_p(ap), int(recs[-1]["str_off"]) + int(recs[-1]["str_len"]))
        words = np.frombuffer(sc.download(C.c_void_p(m.device_segments()[0][0]), k * 8), dtype="<u8")
        for r, w in zip(recs, words.tolist()):
            s = arena[int(r["str_off"]):int(r["str_off"]) + int(r["str_len"])]
            assert w == measure(s), ("Python measures otherwise", s, hex(w), hex(measure(s)))
        lo = int(4.5 * 4096)
        _, sel = timed(lambda: res.select_range_device(m, sx.SX_MEASURE_ENTROPY_SHIFT, 16, lo, 65535))
        random_ones, checked_random = len(sel), int(((words & np.uint64(0xFFFF)) >= np.uint64(lo)).sum())
        sel.free()
        _, sel = timed(lambda: res.select_device(CANNOT_OCCUR, invert=True))
        assert len(sel) == findings
        sel.free(); m.free()
        bufs = []
        download_pinned(sc, res, bufs)
        times = {k: [] for k in ("measure", "everything", "entropy", "download")}
        for _ in range(reps):
            dt, m = timed(res.measure_device)
            times["measure"].append(dt)
            dt, sel = timed(lambda: res.select_range_device(m, sx.SX_MEASURE_ENTROPY_SHIFT, 16, lo, 65535))
            times["entropy"].append(dt)
            sel.free(); m.free()
            dt, sel = timed(lambda: res.select_device(CANNOT_OCCUR, invert=True))
            times["everything"].append(dt)
            sel.free()
            times["download"].append(timed(lambda: download_pinned(sc, res, bufs))[0])
        res.free()
        row = dict(tool="gpu_measure", gib=gib, missions="c5", reps=reps, findings=findings, segments=n_segs, string_bytes=str_bytes, info=info,
                   checked=k, checked_at_4_5_bits=checked_random, at_4_5_bits=random_ones, pinned=PINNED["pinned"], **{k + "_ms": stat(v) for k, v in times.items()})
        sc.free(d); sc.close()
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
