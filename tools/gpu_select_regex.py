"""The selection by compiled regular expressions on the device (sx_select_regex_create / sx_result_select_regex_device) against its
yardsticks: BASELINE config 5's Missions on GIB GiB of background, as tools/gpu_select_set.py.
usage: tools/gpu_select_regex.py [--reps N] [--out FILE] [GIB ...]      (default: 4 16; profiler off)
After a warm-up of every path, alternating, N times each (default 5), the host clock around a call that ends synchronised:
  list16     sx_result_select_device with tools/gpu_select.py's 16 patterns of 4 bytes: the parent's code on the same result
  set16      sx_result_select_set_device with a set of those 16 patterns: the parent's code as well, and re16's yardstick
  re16       sx_result_select_regex_device with the same 16 patterns, escaped: the same automaton as set16's
  re_shapes  ... with six patterns of the kind people grep for in one set: a URL scheme, a dotted quad, an e-mail shape, a
             card-number shape, a `^`-anchored path and a `$`-anchored extension
  fetch      a fresh scan, then every segment fetched to the host: the floor under any search on the host (the scan is not timed)
Checked once, outside the timed region: re16 selects as many findings as set16 and list16; of re_shapes, Python's re agrees on
the first 2 000 selected strings and on the first 2 000 strings of the source.  One JSON line per size (stdout, and appended to
FILE) with the sets' info and the time the compilers took.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` with `--reps 2 4`, a run of its own: per timed repetition the
launches are select_match_kernel (list16), selset_match_kernel (set16), then selre_match_kernel twice (re16, re_shapes)."""
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

SHAPES = [rb"[a-z]{2,6}://", rb"[0-9]{1,3}\.[0-9]{1,3}\.[0-9]{1,3}\.[0-9]{1,3}", rb"[A-Za-z0-9._]+@[A-Za-z0-9]+\.[a-z]{2}",
          rb"[0-9]{4}[ -]?[0-9]{4}", rb"^[A-Z]:\\|^/[a-z]+/", rb"\.(?:exe|dll|[a-z]{2}[0-9])$"]


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
    sx.lib().sx_result_segment_packed.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.POINTER(C.c_uint8)),
                                                  C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(sx.SegmentInfo)]
    shapes_py = [re.compile(p.replace(b"$", b"\\Z")) for p in SHAPES]      # (no SHAPES pattern holds an escaped or bracketed `$`)
    for gib in [float(a) for a in args] or [4, 16]:
        total = int(gib * (1 << 30)) // 4096 * 4096
        sc = sx.Scanner(ms, device=0, result_on_device=True)
        d = sc.alloc(total)
        sc.fill_background(d, 0, total, SEED)

        def scan():
            sc.reset()
            res = sc.scan_device(d, total, file_id=1)
            assert all(s[0] is not None for s in res.device_segments())
            return res

        def select(res, patterns):
            t0 = time.perf_counter()
            sel = res.select_device(patterns)
            dt = (time.perf_counter() - t0) * 1e3
            n = len(sel)
            sel.free()
            return dt, n

        def fetch(res):
            t0 = time.perf_counter()
            for i in range(len(res.device_segments())):
                fp, n, ap, alen, pk = C.c_void_p(), C.c_uint64(), C.POINTER(C.c_uint8)(), C.c_uint64(), C.c_int()
                sc._chk(sx.lib().sx_result_segment_packed(res.h, i, C.byref(fp), C.byref(n), C.byref(ap), C.byref(alen), C.byref(pk), None))
            return (time.perf_counter() - t0) * 1e3

        def strings_of(seg, count):
            """the first `count` strings of a packed device segment"""
            sfp, sn, sap, salen, spk, _ = seg
            assert spk
            recs = np.frombuffer(sc.download(C.c_void_p(sfp), min(sn, count) * 16), dtype=F16)
            if not len(recs):
                return []
            end = int(recs[-1]["str_off"]) + int(recs[-1]["str_len"])
            arena = sc.download(C.c_void_p(sap), end)
            return [arena[int(r["str_off"]):int(r["str_off"]) + int(r["str_len"])] for r in recs]

        res = scan()
        segs = res.device_segments()
        findings, str_bytes, n_segs = len(res), sum(s[3] for s in segs), len(segs)
        fp, n0, ap, alen, packed, _ = segs[0]
        assert packed
        sixteen = []                                            # (tools/gpu_select.py's: the middle 4 bytes of 16 strings)
        for k in range(16):
            r = np.frombuffer(sc.download(C.c_void_p(fp + (k * n0 // 16) * 16), 16), dtype=F16)[0]
            ln = min(int(r["str_len"]), 4)
            sixteen.append(sc.download(C.c_void_p(ap + int(r["str_off"]) + (int(r["str_len"]) - ln) // 2), ln))
        paths, built = {"list16": sixteen}, {}
        for name, make in (("set16", lambda: sc.pattern_set(sixteen)), ("re16", lambda: sc.regex_set([re.escape(p) for p in sixteen])),
                           ("re_shapes", lambda: sc.regex_set(SHAPES))):
            t0 = time.perf_counter()
            paths[name] = make()
            built[name] = round((time.perf_counter() - t0) * 1e3, 2)
        # warm-up of all paths, and the checks
        selected = {name: select(res, p)[1] for name, p in paths.items()}
        assert selected["re16"] == selected["set16"] == selected["list16"], "the regex set, the pattern set and the list select different numbers of findings"
        sel = res.select_device(paths["re_shapes"])
        if len(sel):
            for s in strings_of(sel.device_segments()[0], 2000):
                assert any(r.search(s) for r in shapes_py), "a selected string matches no pattern"
        first = strings_of(segs[0], 2000)
        sel_first = sum(1 for s in first if any(r.search(s) for r in shapes_py))
        if len(sel):
            got = strings_of(sel.device_segments()[0], sel_first)
            assert got == [s for s in first if any(r.search(s) for r in shapes_py)], "Python's re selects other strings"
        sel.free()
        fetch(res)
        res.free()
        times = {k: [] for k in ("list16", "set16", "re16", "re_shapes", "fetch")}
        for _ in range(reps):
            res = scan()
            for name, p in paths.items():
                times[name].append(select(res, p)[0])
            res.free()
            res = scan()
            times["fetch"].append(fetch(res))
            res.free()
        med = {k: stat(v)["median"] for k, v in times.items()}
        row = dict(tool="gpu_select_regex", gib=gib, missions="c5", reps=reps, findings=findings, segments=n_segs, string_bytes=str_bytes,
                   selected=selected, info={k: paths[k].info() for k in ("set16", "re16", "re_shapes")}, create_ms=built,
                   **{k + "_ms": stat(v) for k, v in times.items()},
                   re16_over_set16=round(med["re16"] / med["set16"], 2), fetch_over_re_shapes=round(med["fetch"] / med["re_shapes"], 1),
                   re16_vs_set16="faster" if max(times["re16"]) < min(times["set16"]) else "slower" if min(times["re16"]) > max(times["set16"]) else "not shown",
                   faster_than_fetch="shown" if min(times["fetch"]) > max(times["re16"] + times["re_shapes"]) else "not shown")
        for k in ("set16", "re16", "re_shapes"):
            paths[k].free()
        sc.free(d); sc.close()
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
