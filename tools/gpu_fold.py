"""The Unicode case fold of a device-resident result (sx_result_fold_device) against its yardsticks: BASELINE config 5's Missions on
GIB GiB of background, as tools/gpu_distinct.py.
usage: tools/gpu_fold.py [--reps N] [--out FILE] [GIB ...]      (default: 4; profiler off)
After a warm-up of every path, alternating, N times each (default 5), the host clock around calls that end synchronised:
  fold        one sx_result_fold_device call: a new result with the folded strings, with sx_fold_info
  everything  sx_result_select_device with a pattern that cannot occur, inverted: the whole part selected and gathered —
              result_gather_kernel's time on it is the yardstick of DESIGN.md §7 item 7
  download    the records and the strings of every segment copied to the host (sx_device_download) into pinned memory, as
              tools/gpu_order.py copies them: what a host that folds needs first; download_pageable: the same into Python bytes
  rebind      sx_labels_rebind of the source's distinct words onto the fold
Checked once, outside the timed region: the strings of the first 200 000 findings of segment 0, folded in Python — str.casefold() and
str.lower() per character, as the rule is stated — are the fold's strings, every other byte of their records is the source's, and
sx_fold_info's bytes are the segments' bytes.  One JSON line per size (stdout, and appended to FILE).
Kernel times: run this under `rocprofv3 --kernel-trace --stats` with `--reps 2 4`, a run of its own: per call and segment the launches
are fold_measure_kernel, rocprim's scan and fold_place_kernel."""
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


def fold_char(x):
    if 0xD800 <= ord(x) <= 0xDFFF:
        return x
    f = x.casefold()
    if len(f) == 1:
        return f
    f = x.lower()
    return f if len(f) == 1 else x


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
    table = {c: fold_char(chr(c)) for c in range(0x110000) if fold_char(chr(c)) != chr(c)}
    ms = sx.missions_from_flags(**C5)
    for gib in [float(a) for a in args] or [4]:
        total = int(gib * (1 << 30)) // 4096 * 4096
        sc = sx.Scanner(ms, device=0, result_on_device=True)
        d = sc.alloc(total)
        sc.fill_background(d, 0, total, SEED)

        def scan():
            sc.reset()
            res = sc.scan_device(d, total, file_id=1)
            assert all(s[0] is not None for s in res.device_segments())
            return res

        def timed(call):
            t0 = time.perf_counter()
            got = call()
            return (time.perf_counter() - t0) * 1e3, got

        def download(res):
            return [(sc.download(C.c_void_p(fp), n * (16 if packed else 32)), sc.download(C.c_void_p(ap), alen)) for fp, n, ap, alen, packed, _ in res.device_segments()]

        # warm-up of all paths, and the checks
        res = scan()
        segs = res.device_segments()
        findings, str_bytes, n_segs = len(res), sum(s[3] for s in segs), len(segs)
        _, fold = timed(res.fold_device)
        info = fold.fold_info
        fsegs = fold.device_segments()
        assert [(s[1], s[4]) for s in fsegs] == [(s[1], s[4]) for s in segs] and info["findings"] == findings and info["bytes_out"] == sum(s[3] for s in fsegs), (info, fsegs)
        (fp, n0, ap, _, packed, _), (ffp, _, fap, _, _, _) = segs[0], fsegs[0]
        assert packed
        k = min(n0, 200_000)
        recs, frecs = (np.frombuffer(sc.download(C.c_void_p(p), k * 16), dtype=F16) for p in (fp, ffp))
        arena, farena = (sc.download(C.c_void_p(p), int(r[-1]["str_off"]) + int(r[-1]["str_len"])) for p, r in ((ap, recs), (fap, frecs)))
        changed = 0
        for r, f in zip(recs, frecs):
            s = arena[int(r["str_off"]):int(r["str_off"]) + int(r["str_len"])]
            g = farena[int(f["str_off"]):int(f["str_off"]) + int(f["str_len"])]
            want = s.decode("utf-8", "surrogateescape").translate(table).encode("utf-8", "surrogateescape")
            assert g == want and (r["position"], r["flags"], r["mission_id"]) == (f["position"], f["flags"], f["mission_id"]), ("Python folds otherwise", s, g, want)
            changed += g != s
        lab = res.distinct_device()
        _, bound = timed(lambda: lab.rebind(fold))
        bound.free()
        _, sel = timed(lambda: res.select_device(CANNOT_OCCUR, invert=True))
        assert len(sel) == findings
        sel.free(); fold.free()
        download(res)
        bufs = []
        download_pinned(sc, res, bufs)
        times = {k: [] for k in ("fold", "everything", "download", "download_pageable", "rebind")}
        for _ in range(reps):
            dt, fold = timed(res.fold_device)
            times["fold"].append(dt)
            dt, bound = timed(lambda: lab.rebind(fold))
            times["rebind"].append(dt)
            bound.free(); fold.free()
            dt, sel = timed(lambda: res.select_device(CANNOT_OCCUR, invert=True))
            times["everything"].append(dt)
            sel.free()
            times["download"].append(timed(lambda: download_pinned(sc, res, bufs))[0])
            times["download_pageable"].append(timed(lambda: download(res))[0])
        lab.free(); res.free()
        row = dict(tool="gpu_fold", gib=gib, missions="c5", reps=reps, findings=findings, segments=n_segs, string_bytes=str_bytes, info=info,
                   checked=k, checked_changed=int(changed), pinned=PINNED["pinned"], **{k + "_ms": stat(v) for k, v in times.items()})
        sc.free(d); sc.close()
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
