"""A seen set that counts (SX_SEEN_COUNTED, sx_result_seen_counts_device, sx_result_select_labels_range_device) against its
yardsticks: BASELINE config 5's Missions on GIB GiB of background, as tools/gpu_seen.py, a plain set and a counted set side by side.
usage: tools/gpu_seen_counts.py [--reps N] [--out FILE] [GIB ...]      (default: 4; profiler off)
After a warm-up of every path, alternating, N times each (default 5), the host clock around calls that end synchronised:
  plain_empty / plain_full      sx_result_seen_device into an EMPTY plain set (reset in front of it, untimed), and the same call again:
                                tools/gpu_seen.py's seen_empty and seen_full — what the parent commit's numbers are compared with
  counted_empty / counted_full  the same two calls into a set that counts: the add pass and seen_count_kernel, then seen_count_kernel alone
  counts_lookup                 sx_result_seen_counts_device: seen_counts_lookup_kernel once per segment, no distinct pass
  range_select                  sx_result_select_labels_range_device(count words, results >= 2): label_range_pick_kernel as pass 1
  merge_counted                 sx_seen_set_merge of the counted set into an empty counted set of the same capacity: the merge's mark
                                and add passes and seen_merge_count_kernel
  everything                    sx_result_select_labels_device(words) with no mask: the whole part gathered — result_gather_kernel's
                                time on it is the yardstick of DESIGN.md §7 item 7
Checked once, outside the timed region: the counted set's words and info are the plain set's; after the two calls every string's
count is (2, twice its class) — read through the count words of segment 0 against the distinct words —; the range selection keeps
every finding; the merged set holds the source's strings.  One JSON line per size (stdout, and appended to FILE).
Kernel times: run this under `rocprofv3 --kernel-trace --stats` with `--reps 2 4`, a run of its own."""
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
            x = call()
            return (time.perf_counter() - t0) * 1e3, x

        def words0(res, lab):
            return np.frombuffer(sc.download(C.c_void_p(lab.device_segments()[0][0]), res.device_segments()[0][1] * 8), dtype="<u8")

        # warm-up of all paths, and the checks
        res = scan()
        segs = res.device_segments()
        findings, str_bytes, n_segs = len(res), sum(s[3] for s in segs), len(segs)
        lab = res.distinct_device()
        info = lab.info
        room = (info["distinct"], str_bytes + 15 * info["distinct"])
        plain, counted, merged = sc.seen_set(*room), sc.seen_set(*room, counted=True), sc.seen_set(*room, counted=True)
        pe, ce = res.seen_device(plain), res.seen_device(counted)
        pf, cf = res.seen_device(plain), res.seen_device(counted)
        assert pe.info == ce.info and pf.info == cf.info and plain.info() == counted.info(), (pe.info, ce.info)
        assert np.array_equal(words0(res, pe), words0(res, ce)) and np.array_equal(words0(res, pf), words0(res, cf))
        cw = res.seen_counts_device(counted)
        dw, got = words0(res, lab), words0(res, cw)
        size = dw >> np.uint64(sx.SX_DISTINCT_COUNT_SHIFT)      # (the classes of this source are far from 2^31 members)
        assert np.array_equal(got, (np.uint64(2) * size) << np.uint64(sx.SX_SEEN_FINDINGS_SHIFT) | np.uint64(2) << np.uint64(sx.SX_SEEN_RESULTS_SHIFT))
        sel = res.select_range_device(cw, sx.SX_SEEN_RESULTS_SHIFT, 32, 2, (1 << 32) - 1)
        assert len(sel) == findings
        sel.free()
        mi = merged.merge(counted)
        assert mi["source_strings"] == mi["added_strings"] == info["distinct"] and merged.info()["strings"] == info["distinct"], mi
        for x in (lab, pe, ce, pf, cf, cw):
            x.free()
        res.free()
        names = ("plain_empty", "plain_full", "counted_empty", "counted_full", "counts_lookup", "range_select", "merge_counted", "everything")
        times = {k: [] for k in names}
        for _ in range(reps):
            res = scan()
            lab = res.distinct_device()
            labs = [lab]
            for name, ss in (("plain", plain), ("counted", counted)):
                ss.reset()
                for which in ("empty", "full"):
                    dt, x = timed(lambda: res.seen_device(ss))
                    times["%s_%s" % (name, which)].append(dt)
                    labs.append(x)
            dt, cw = timed(lambda: res.seen_counts_device(counted))
            times["counts_lookup"].append(dt)
            labs.append(cw)
            dt, sel = timed(lambda: res.select_range_device(cw, sx.SX_SEEN_RESULTS_SHIFT, 32, 2, (1 << 32) - 1))
            times["range_select"].append(dt)
            sel.free()
            merged.reset()
            times["merge_counted"].append(timed(lambda: merged.merge(counted))[0])
            dt, sel = timed(lambda: res.select_device(lab))
            times["everything"].append(dt)
            sel.free()
            for x in labs:
                x.free()
            res.free()
        row = dict(tool="gpu_seen_counts", gib=gib, missions="c5", reps=reps, findings=findings, segments=n_segs, string_bytes=str_bytes, info=info,
                   set=counted.info(), **{k + "_ms": stat(v) for k, v in times.items()})
        for ss in (plain, counted, merged):
            ss.free()
        sc.free(d); sc.close()
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
