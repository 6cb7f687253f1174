"""The labels of a device-resident result (sx_label_set_create / sx_result_label_device / sx_result_select_labels_device) against
their yardsticks: BASELINE config 5's Missions on GIB GiB of background, as tools/gpu_select_regex.py, with its six re_shapes patterns.
usage: tools/gpu_label.py [--reps N] [--out FILE] [GIB ...]      (default: 4; profiler off)
After a warm-up of every path, alternating, N times each (default 5), the host clock around calls that end synchronised:
  label6   one sx_result_label_device call with a label set of the six patterns: which of them every finding holds, and the count
  sel6x1   the parent's way to the same information: six sx_result_select_regex_device calls with a regex set of one pattern each
  re6      one sx_result_select_regex_device call with the six in one regex set: the one-bit answer
  pick     sx_result_select_labels_device(labels, any = 1): the findings that hold pattern 0, by their labels
  re1      sx_result_select_regex_device with pattern 0 alone: the same findings, by a walk over the strings
Checked once, outside the timed region: per pattern the set's count of findings equals the number the one-pattern regex selection
selects; `pick` selects as many as `re1`; Python's re agrees with the labels of the first 2 000 findings of segment 0.  One JSON
line per size (stdout, and appended to FILE) with the sets' info and the time the compilers took.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` with `--reps 2 4`, a run of its own: per timed repetition the
launches are label_match_kernel (label6), selre_match_kernel seven times (sel6x1, re6), label_pick_kernel (pick), selre_match_kernel
(re1), each per segment."""
import ctypes as C
import json
import os
import re
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import stringsext_amd as sx
from gpu_select import C5, F16, SEED, stat
from gpu_select_regex import SHAPES


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
    shapes_py = [re.compile(p.replace(b"$", b"\\Z")) for p in SHAPES]      # (no SHAPES pattern holds an escaped or bracketed `$`)
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

        def select(res, how, **masks):
            t0 = time.perf_counter()
            sel = res.select_device(how, **masks)
            dt = (time.perf_counter() - t0) * 1e3
            n = len(sel)
            sel.free()
            return dt, n

        def label(res, keep=False):
            t0 = time.perf_counter()
            lab = res.label_device(ls)
            dt = (time.perf_counter() - t0) * 1e3
            if keep:
                return dt, lab
            lab.free()
            return dt, None

        built = {}
        t0 = time.perf_counter()
        ls = sc.label_set(SHAPES)
        built["label6"] = round((time.perf_counter() - t0) * 1e3, 2)
        t0 = time.perf_counter()
        ones = [sc.regex_set([p]) for p in SHAPES]
        built["sel6x1"] = round((time.perf_counter() - t0) * 1e3, 2)
        t0 = time.perf_counter()
        six = sc.regex_set(SHAPES)
        built["re6"] = round((time.perf_counter() - t0) * 1e3, 2)
        # warm-up of all paths, and the checks
        res = scan()
        segs = res.device_segments()
        findings, str_bytes, n_segs = len(res), sum(s[3] for s in segs), len(segs)
        _, lab = label(res, keep=True)
        counted = ls.read()[0]
        by_regex = [select(res, r)[1] for r in ones]
        assert counted == by_regex, ("the label set's counts and the one-pattern regex selections differ", counted, by_regex)
        selected = dict(per_pattern=counted, re6=select(res, six)[1], pick=select(res, lab, any=1)[1])
        assert selected["pick"] == by_regex[0], "the pick by label and the regex selection of pattern 0 select different numbers of findings"
        fp, n0, ap, _, packed, _ = segs[0]
        assert packed
        k = min(n0, 2000)
        recs = np.frombuffer(sc.download(C.c_void_p(fp), k * 16), dtype=F16)
        arena = sc.download(C.c_void_p(ap), int(recs[-1]["str_off"]) + int(recs[-1]["str_len"]))
        words = np.frombuffer(sc.download(C.c_void_p(lab.device_segments()[0][0]), k * 8), dtype="<u8")
        for r, w in zip(recs, words):
            s = arena[int(r["str_off"]):int(r["str_off"]) + int(r["str_len"])]
            assert int(w) == sum(1 << p for p, x in enumerate(shapes_py) if x.search(s)), ("Python's re labels a string otherwise", s, hex(int(w)))
        lab.free(); res.free()
        times = {k: [] for k in ("label6", "sel6x1", "re6", "pick", "re1")}
        for _ in range(reps):
            res = scan()
            dt, lab = label(res, keep=True)
            times["label6"].append(dt)
            times["sel6x1"].append(sum(select(res, r)[0] for r in ones))
            times["re6"].append(select(res, six)[0])
            times["pick"].append(select(res, lab, any=1)[0])
            times["re1"].append(select(res, ones[0])[0])
            lab.free(); res.free()
        med = {k: stat(v)["median"] for k, v in times.items()}
        i = ls.info
        row = dict(tool="gpu_label", gib=gib, missions="c5", reps=reps, findings=findings, segments=n_segs, string_bytes=str_bytes, selected=selected,
                   info=dict(label6={k: getattr(i, k) for k, _ in sx.LabelSetInfo._fields_}, re6=six.info(), re1=ones[0].info()), create_ms=built,
                   **{k + "_ms": stat(v) for k, v in times.items()},
                   sel6x1_over_label6=round(med["sel6x1"] / med["label6"], 2), label6_over_re6=round(med["label6"] / med["re6"], 2),
                   re1_over_pick=round(med["re1"] / med["pick"], 2),
                   label6_vs_sel6x1="faster" if max(times["label6"]) < min(times["sel6x1"]) else "slower" if min(times["label6"]) > max(times["sel6x1"]) else "not shown",
                   pick_vs_re1="faster" if max(times["pick"]) < min(times["re1"]) else "slower" if min(times["pick"]) > max(times["re1"]) else "not shown")
        for x in ones + [six, ls]:
            x.free()
        sc.free(d); sc.close()
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
