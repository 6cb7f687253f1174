"""A seen set's merge kernels (sx_seen_set_merge, sx_seen_set_grow) against their yardsticks: BASELINE config 5's Missions on GIB GiB
of background, the part of tools/gpu_seen.py.
usage: tools/gpu_seen_merge.py [--reps N] [--out FILE] [GIB ...]      (default: 4; profiler off)
After a warm-up of every path, alternating, N times each (default 5), the host clock around calls that end synchronised:
  seen_empty  sx_result_seen_device into an EMPTY set (reset in front of it, untimed): the parent's seen_add_kernel on these entries
  grow        sx_seen_set_grow of the full set to twice its capacity: the new set's memory allocated and emptied, every entry looked
              up in an empty table (seen_merge_mark_kernel) and copied and claimed (seen_merge_add_kernel); the old memory freed
  shrink      sx_seen_set_grow back to the capacity it had (untimed paths alike; it puts the set back for the next round)
  merge_new   sx_seen_set_merge of the full set into an EMPTY second set of the same capacity: the two kernels without the allocation
  merge_held  the same call again: the second set holds everything — every lookup compares an entry to its end, nothing is added
  everything  sx_result_select_labels_device(words) with no mask: the whole part gathered — result_gather_kernel's time on it is the
              yardstick of DESIGN.md §7 item 7
Checked once, outside the timed region: the grown set holds what it held, under a table one bit larger; merge_new adds every string
and merge_held none; a lookup of the result in the second set sees every finding.  One JSON line per size (stdout, and appended to
FILE).  Kernel times: run this under `rocprofv3 --kernel-trace --stats` with `--reps 2 4`, a run of its own: per grow, shrink and
merge_new one seen_merge_mark_kernel and one seen_merge_add_kernel, per merge_held one seen_merge_mark_kernel."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

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

        def timed(call):
            t0 = time.perf_counter()
            got = call()
            return (time.perf_counter() - t0) * 1e3, got

        def select(res, lab):
            t0 = time.perf_counter()
            sel = res.select_device(lab)
            dt = (time.perf_counter() - t0) * 1e3
            n = len(sel)
            sel.free()
            return dt, n

        sc.reset()
        res = sc.scan_device(d, total, file_id=1)
        segs = res.device_segments()
        assert all(s[0] is not None for s in segs)
        findings, str_bytes = len(res), sum(s[3] for s in segs)
        lab = res.distinct_device()
        distinct = lab.info["distinct"]
        cap_s, cap_b = distinct, str_bytes + 15 * distinct
        ss, other = sc.seen_set(cap_s, cap_b), sc.seen_set(cap_s, cap_b)
        times = {k: [] for k in ("seen_empty", "grow", "shrink", "merge_new", "merge_held", "everything")}
        infos = {}
        for rep in range(reps + 1):                  # (the first round is the warm-up, with the checks)
            ss.reset()
            t_empty, empty = timed(lambda: res.seen_device(ss))
            full = ss.info()
            t_grow, _ = timed(lambda: ss.grow(2 * cap_s, 2 * cap_b))
            grown = ss.info()
            t_shrink, _ = timed(lambda: ss.grow(cap_s, cap_b))
            other.reset()
            t_new, m_new = timed(lambda: other.merge(ss))
            t_held, m_held = timed(lambda: other.merge(ss))
            t_all, n_all = select(res, lab)
            if rep == 0:
                assert empty.info["added_strings"] == distinct == full["strings"] and full["bytes"] == empty.info["added_bytes"], (empty.info, full)
                assert (grown["strings"], grown["bytes"], grown["table_log2"]) == (full["strings"], full["bytes"], full["table_log2"] + 1), (full, grown)
                assert ss.info() == full, (ss.info(), full)
                assert m_new == dict(source_strings=distinct, already_held=0, added_strings=distinct, added_bytes=full["bytes"]), m_new
                assert m_held == dict(source_strings=distinct, already_held=distinct, added_strings=0, added_bytes=0), m_held
                looked = res.seen_device(other, add=False)
                assert looked.info["seen_findings"] == findings and looked.info["seen_distinct"] == distinct, looked.info
                looked.free()
                assert n_all == findings
                infos = dict(set=full, grown=grown, merge_new=m_new, merge_held=m_held)
            else:
                for k, v in (("seen_empty", t_empty), ("grow", t_grow), ("shrink", t_shrink), ("merge_new", t_new), ("merge_held", t_held), ("everything", t_all)):
                    times[k].append(v)
            empty.free()
        row = dict(tool="gpu_seen_merge", gib=gib, missions="c5", reps=reps, findings=findings, segments=len(segs), string_bytes=str_bytes, distinct=distinct,
                   **infos, **{k + "_ms": stat(v) for k, v in times.items()})
        lab.free(); res.free(); ss.free(); other.free()
        sc.free(d); sc.close()
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
