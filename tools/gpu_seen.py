"""The seen set of device-resident results (sx_seen_set, sx_result_seen_device) against its yardsticks: BASELINE config 5's Missions
on GIB GiB of background, as tools/gpu_distinct.py.
usage: tools/gpu_seen.py [--reps N] [--out FILE] [GIB ...]      (default: 4; profiler off)
After a warm-up of every path, alternating, N times each (default 5), the host clock around calls that end synchronised:
  distinct    one sx_result_distinct_device call: what every seen call contains
  seen_empty  sx_result_seen_device into an EMPTY set (reset in front of it, untimed): every lookup ends at an empty slot or a
              stranger's tag, every class is added
  seen_full   the same call again: the set holds every string — every lookup compares an entry to its end, nothing is added
  lookup      the same with SX_SEEN_LOOKUP_ONLY
  everything  sx_result_select_labels_device(words) with no mask: the whole part gathered — result_gather_kernel's time on it is the
              yardstick of DESIGN.md §7 item 7
The set's capacity: the result's classes, and its string bytes + 15 per class (an entry is 8 bytes and its string rounded up to 8).
Checked once, outside the timed region: into the empty set every class is added and no finding is seen; afterwards the set holds
`distinct` strings, every finding is seen and nothing is added; the words of segment 0 are the distinct call's plus SX_DISTINCT_SEEN;
a lookup changes nothing.  One JSON line per size (stdout, and appended to FILE).
Kernel times: run this under `rocprofv3 --kernel-trace --stats` with `--reps 2 4`, a run of its own: per seen call the launches are
the distinct call's and seen_mark_kernel once per segment, and seen_add_kernel once per segment where something is new."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import stringsext_amd as sx
from gpu_select import C5, SEED, stat


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

        def scan():
            sc.reset()
            res = sc.scan_device(d, total, file_id=1)
            assert all(s[0] is not None for s in res.device_segments())
            return res

        def timed(call):
            t0 = time.perf_counter()
            lab = call()
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
        _, lab = timed(res.distinct_device)
        info = lab.info
        ss = sc.seen_set(info["distinct"], str_bytes + 15 * info["distinct"])
        _, empty = timed(lambda: res.seen_device(ss))
        info_empty, set_info = empty.info, ss.info()
        assert info_empty["seen_findings"] == 0 and info_empty["added_strings"] == info["distinct"] == set_info["strings"], (info_empty, info, set_info)
        assert set_info["bytes"] == info_empty["added_bytes"] <= set_info["capacity_bytes"]
        _, full = timed(lambda: res.seen_device(ss))
        info_full = full.info
        assert info_full["seen_findings"] == findings and info_full["seen_distinct"] == info["distinct"] and info_full["added_strings"] == 0, info_full
        _, looked = timed(lambda: res.seen_device(ss, add=False))
        assert looked.info == info_full and ss.info() == set_info
        n0 = segs[0][1]
        words = [np.frombuffer(sc.download(C.c_void_p(x.device_segments()[0][0]), n0 * 8), dtype="<u8") for x in (lab, empty, full, looked)]
        assert np.array_equal(words[0], words[1]) and np.array_equal(words[0] | np.uint64(sx.SX_DISTINCT_SEEN), words[2]) and np.array_equal(words[2], words[3])
        selected = dict(new=select(res, empty, any=sx.SX_DISTINCT_FIRST, none=sx.SX_DISTINCT_SEEN)[1], everything=select(res, full)[1])
        assert selected["new"] == info["distinct"] and selected["everything"] == findings, selected
        for x in (lab, empty, full, looked):
            x.free()
        res.free()
        times = {k: [] for k in ("distinct", "seen_empty", "seen_full", "lookup", "everything")}
        for _ in range(reps):
            res = scan()
            dt, lab = timed(res.distinct_device)
            times["distinct"].append(dt)
            ss.reset()
            dt, empty = timed(lambda: res.seen_device(ss))
            times["seen_empty"].append(dt)
            dt, full = timed(lambda: res.seen_device(ss))
            times["seen_full"].append(dt)
            dt, looked = timed(lambda: res.seen_device(ss, add=False))
            times["lookup"].append(dt)
            times["everything"].append(select(res, lab)[0])
            for x in (lab, empty, full, looked):
                x.free()
            res.free()
        row = dict(tool="gpu_seen", gib=gib, missions="c5", reps=reps, findings=findings, segments=n_segs, string_bytes=str_bytes, selected=selected,
                   info=info, info_empty=info_empty, info_full=info_full, set=set_info, **{k + "_ms": stat(v) for k, v in times.items()})
        ss.free()
        sc.free(d); sc.close()
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
