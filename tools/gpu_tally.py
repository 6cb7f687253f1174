"""The keyword tally on the device (sx_tally_set_create / sx_result_tally_device) next to the kernel it was modelled on: BASELINE config
5's Missions on GIB GiB of background, as tools/gpu_select_set.py.
usage: tools/gpu_tally.py [--reps N] [--out FILE] [GIB ...]      (default: 4; profiler off)
After a warm-up of every path, alternating, N times each (default 5), the host clock around a call that ends synchronised:
  tally16 / tally1000 / tally10000     sx_result_tally_device with 16, 1 000 and 10 000 keywords, the middle 4..10 bytes of strings
                                       spread over the result's first segment (tools/gpu_select_set.py's lists)
  walk16 / walk1000 / walk10000        sx_result_select_set_device with SX_SELECT_INVERT and the same lists as DECOYS (a byte 02 in
                                       front of every keyword: none occurs), so selset_match_kernel walks every string to its end as
                                       the tally kernel does; the call also places and gathers every finding, which the tally does not
Checked once, outside the timed region: every keyword has at least one hit and its first ordinal is at most the index of the finding
it was taken from; the decoy sets select every finding.  One JSON line per size (stdout, and appended to FILE) with the sets'
sx_tally_set_info and the time sx_tally_set_create took.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` with `--reps 2 4`, a run of its own: per timed repetition the launches
are seltally_kernel (16, 1 000, 10 000 keywords, one launch per segment each), then selset_match_kernel in the same order."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import stringsext_amd as sx
from gpu_select import C5, F16, SEED, stat


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
        findings, str_bytes = len(res), sum(s[3] for s in segs)
        fp, n0, ap, alen, packed, _ = segs[0]
        assert packed

        def taken(count, length):
            """(keyword, index of the finding it was taken from) of `count` strings spread over the first segment"""
            got = []
            for k in range(count):
                i = k * n0 // count
                r = np.frombuffer(sc.download(C.c_void_p(fp + i * 16), 16), dtype=F16)[0]
                ln = min(int(r["str_len"]), length(k))
                o = int(r["str_off"]) + (int(r["str_len"]) - ln) // 2
                got.append((sc.download(C.c_void_p(ap + o), ln), i))
            return got

        lists = {16: taken(16, lambda k: 4), 1000: taken(1000, lambda k: 4 + k % 7), 10000: taken(10000, lambda k: 4 + k % 7)}
        tallies, walks, built = {}, {}, {}
        for n, source in lists.items():
            t0 = time.perf_counter()
            tallies[n] = sc.tally_set([p for p, _ in source])
            built[f"tally{n}"] = round((time.perf_counter() - t0) * 1e3, 2)
            walks[n] = sc.pattern_set([b"\x02" + p for p, _ in source])

        def tally(n):
            t0 = time.perf_counter()
            walked = res.tally_device(tallies[n])
            dt = (time.perf_counter() - t0) * 1e3
            assert walked == findings
            return dt

        def walk(n):
            t0 = time.perf_counter()
            sel = res.select_device(walks[n], invert=True)
            dt = (time.perf_counter() - t0) * 1e3
            assert len(sel) == findings
            sel.free()
            return dt

        # warm-up of all paths, and the checks
        total_hits = {}
        for n, source in lists.items():
            tally(n); walk(n)
            hits, first = tallies[n].read()
            assert all(h > 0 for h in hits) and all(f <= i for f, (_, i) in zip(first, source)), "a keyword taken from a string was not counted there"
            total_hits[f"tally{n}"] = sum(hits)
            tallies[n].reset()
        times = {f"{what}{n}": [] for what in ("tally", "walk") for n in lists}
        for _ in range(reps):
            for n in lists:
                times[f"tally{n}"].append(tally(n))
            for n in lists:
                times[f"walk{n}"].append(walk(n))
        row = dict(tool="gpu_tally", gib=gib, missions="c5", reps=reps, findings=findings, segments=len(segs), string_bytes=str_bytes,
                   hits=total_hits, set_info={f"tally{n}": t.info() for n, t in tallies.items()}, set_create_ms=built,
                   **{k + "_ms": stat(v) for k, v in times.items()})
        for t in list(tallies.values()) + list(walks.values()):
            t.free()
        res.free()
        sc.free(d); sc.close()
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
