"""The duplicate strings of a device-resident result (sx_result_distinct_device) against their yardstick: BASELINE config 5's Missions
on GIB GiB of background, as tools/gpu_label.py.
usage: tools/gpu_distinct.py [--reps N] [--out FILE] [--dominant N] [GIB ...]      (default: 4; profiler off)
After a warm-up of every path, alternating, N times each (default 5), the host clock around calls that end synchronised:
  distinct   one sx_result_distinct_device call: a word per finding, with info's rounds and table_log2
  folded     the same with SX_SELECT_ASCII_NOCASE
  sort_u     sx_result_select_labels_device(words, any = SX_DISTINCT_FIRST): the first of every class, by the words
  everything sx_result_select_labels_device(words) with no mask: the whole part gathered — result_gather_kernel's time on it is the
             yardstick of DESIGN.md §7 item 7
--dominant N: the first N x 32 bytes of the buffer are N copies of one 31-byte line: what N adds to one `count` word cost.
Checked once, outside the timed region: a Python dict over the strings of the first 200 000 findings of segment 0 agrees with the
FIRST bits of their words (a finding without an equal in front of it among them has none in the result), sort_u selects info's
`distinct` findings.  One JSON line per size (stdout, and appended to FILE), with the size of segment 0's largest class (with
--dominant N: at least N if the Missions find the planted line whole).
The findings left after each round: run with SX_TIMING=1, the library writes a line per round to stderr.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` with `--reps 2 4`, a run of its own: per call the launches are
distinct_claim_kernel and distinct_resolve_kernel once per round and segment, distinct_finalize_kernel once per segment."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import stringsext_amd as sx
from gpu_select import C5, F16, SEED, stat

LINE = b"one-line-planted-again-and-again"[:31] + b"\x00"


def main():
    args, reps, out, dominant = sys.argv[1:], 5, None, 0
    while args and args[0].startswith("--"):
        if args[0] == "--reps":
            reps = int(args[1])
        elif args[0] == "--out":
            out = args[1]
        elif args[0] == "--dominant":
            dominant = int(args[1])
        else:
            sys.exit(__doc__)
        args = args[2:]
    ms = sx.missions_from_flags(**C5)
    for gib in [float(a) for a in args] or [4]:
        total = int(gib * (1 << 30)) // 4096 * 4096
        sc = sx.Scanner(ms, device=0, result_on_device=True)
        d = sc.alloc(total)
        sc.fill_background(d, 0, total, SEED)
        if dominant:
            assert dominant * len(LINE) <= total
            sc.upload(d, LINE * dominant)

        def scan():
            sc.reset()
            res = sc.scan_device(d, total, file_id=1)
            assert all(s[0] is not None for s in res.device_segments())
            return res

        def distinct(res, fold=False):
            t0 = time.perf_counter()
            lab = res.distinct_device(ignore_case=fold)
            return (time.perf_counter() - t0) * 1e3, lab

        def select(res, lab, **masks):
            t0 = time.perf_counter()
            sel = res.select_device(lab, **masks)
            dt = (time.perf_counter() - t0) * 1e3
            n = len(sel)
            sel.free()
            return dt, n

        # warm-up of all paths, and the checks
        res = scan()
        segs = res.device_segments()
        findings, str_bytes, n_segs = len(res), sum(s[3] for s in segs), len(segs)
        _, lab = distinct(res)
        info = lab.info
        _, folded = distinct(res, fold=True)
        info_folded = folded.info
        folded.free()
        selected = dict(sort_u=select(res, lab, any=sx.SX_DISTINCT_FIRST)[1], everything=select(res, lab)[1])
        assert selected["sort_u"] == info["distinct"] and selected["everything"] == findings == info["findings"], (selected, info)
        fp, n0, ap, _, packed, _ = segs[0]
        assert packed
        k = min(n0, 200_000)
        recs = np.frombuffer(sc.download(C.c_void_p(fp), k * 16), dtype=F16)
        arena = sc.download(C.c_void_p(ap), int(recs[-1]["str_off"]) + int(recs[-1]["str_len"]))
        words = np.frombuffer(sc.download(C.c_void_p(lab.device_segments()[0][0]), n0 * 8), dtype="<u8")
        seen = set()
        for r, w in zip(recs, words[:k]):
            s = arena[int(r["str_off"]):int(r["str_off"]) + int(r["str_len"])]
            assert bool(int(w) & sx.SX_DISTINCT_FIRST) == (s not in seen), ("a Python dict says otherwise", s, hex(int(w)))
            seen.add(s)
        largest = int((words >> np.uint64(sx.SX_DISTINCT_COUNT_SHIFT)).max())
        lab.free(); res.free()
        times = {k: [] for k in ("distinct", "folded", "sort_u", "everything")}
        for _ in range(reps):
            res = scan()
            dt, lab = distinct(res)
            times["distinct"].append(dt)
            dt, folded = distinct(res, fold=True)
            times["folded"].append(dt)
            folded.free()
            times["sort_u"].append(select(res, lab, any=sx.SX_DISTINCT_FIRST)[0])
            times["everything"].append(select(res, lab)[0])
            lab.free(); res.free()
        row = dict(tool="gpu_distinct", gib=gib, missions="c5", reps=reps, dominant=dominant, findings=findings, segments=n_segs, string_bytes=str_bytes,
                   selected=selected, largest_class=largest, info=info, info_folded=info_folded, **{k + "_ms": stat(v) for k, v in times.items()})
        sc.free(d); sc.close()
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
