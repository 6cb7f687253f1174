"""The selection by a compiled keyword list on the device (sx_select_set_create / sx_result_select_set_device) against its two yardsticks:
BASELINE config 5's Missions on GIB GiB of background, as tools/gpu_select.py.
usage: tools/gpu_select_set.py [--reps N] [--out FILE] [GIB ...]      (default: 4 16; profiler off)
After a warm-up of every path, alternating, N times each (default 5), the host clock around a call that ends synchronised:
  list16    sx_result_select_device with tools/gpu_select.py's 16 patterns of 4 bytes: the parent's code on the same result
  set16     sx_result_select_set_device with a set of those 16 patterns
  set1000   ... with 1 000 keywords, the middle 4..10 bytes of strings spread over the result's first segment
  set10000  ... with 10 000 of them
  fetch     a fresh scan, then every segment fetched to the host: the floor under any search on the host (the scan is not timed)
Checked once, outside the timed region: set16 selects as many findings as list16; of each keyword set, every selected string of
the first 2 000 holds a keyword and every string a keyword was taken from is selected.  One JSON line per size (stdout, and
appended to FILE) with the sets' sx_select_set_info and the time sx_select_set_create took.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` with `--reps 2 4`, a run of its own: per timed repetition the
launches are select_match_kernel (list16), then selset_match_kernel three times (set16, set1000, set10000), in this order."""
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
    sx.lib().sx_result_segment_packed.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.POINTER(C.c_uint8)),
                                                  C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.POINTER(sx.SegmentInfo)]
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

        res = scan()
        segs = res.device_segments()
        findings, str_bytes, n_segs = len(res), sum(s[3] for s in segs), len(segs)
        rec_bytes = sum(s[1] * (16 if s[4] else 32) for s in segs)
        fp, n0, ap, alen, packed, _ = segs[0]
        assert packed

        def taken(count, length):
            """(keyword, position of the finding it was taken from) of `count` strings spread over the first segment"""
            got = []
            for k in range(count):
                r = np.frombuffer(sc.download(C.c_void_p(fp + (k * n0 // count) * 16), 16), dtype=F16)[0]
                ln = min(int(r["str_len"]), length(k))
                o = int(r["str_off"]) + (int(r["str_len"]) - ln) // 2
                got.append((sc.download(C.c_void_p(ap + o), ln), int(r["position"])))
            return got

        sixteen = [p for p, _ in taken(16, lambda k: 4)]        # (tools/gpu_select.py's)
        sets, built = {}, {}
        for name, source in (("set16", [(p, None) for p in sixteen]), ("set1000", taken(1000, lambda k: 4 + k % 7)), ("set10000", taken(10000, lambda k: 4 + k % 7))):
            t0 = time.perf_counter()
            ps = sc.pattern_set([p for p, _ in source])
            built[name] = round((time.perf_counter() - t0) * 1e3, 2)
            sets[name] = (ps, source)
        # warm-up of all paths, and the checks
        _, n_list16 = select(res, sixteen)
        selected = {}
        for name, (ps, source) in sets.items():
            sel = res.select_device(ps)
            selected[name] = len(sel)
            if name == "set16":
                assert len(sel) == n_list16, "the set and the list select different numbers of findings"
            else:
                sfp, sn, sap, salen, spk, _ = sel.device_segments()[0]
                recs = np.frombuffer(sc.download(C.c_void_p(sfp), sn * 16), dtype=F16)
                strings = sc.download(C.c_void_p(sap), salen)
                keywords = [p for p, _ in source]
                for r in recs[:2000]:
                    s = strings[int(r["str_off"]):int(r["str_off"]) + int(r["str_len"])]
                    assert any(p in s for p in keywords), "a selected string holds no keyword"
                assert {pos for _, pos in source} <= set(recs["position"].tolist()), "a string a keyword was taken from is not selected"
            sel.free()
        fetch(res)
        res.free()
        times = {k: [] for k in ("list16", "set16", "set1000", "set10000", "fetch")}
        for _ in range(reps):
            res = scan()
            times["list16"].append(select(res, sixteen)[0])
            for name, (ps, _) in sets.items():
                times[name].append(select(res, ps)[0])
            res.free()
            res = scan()
            times["fetch"].append(fetch(res))
            res.free()
        med = {k: stat(v)["median"] for k, v in times.items()}
        row = dict(tool="gpu_select_set", gib=gib, missions="c5", reps=reps, findings=findings, segments=n_segs, string_bytes=str_bytes,
                   record_bytes=rec_bytes, selected_list16=n_list16, selected=selected, set_info={k: v[0].info() for k, v in sets.items()},
                   set_create_ms=built, **{k + "_ms": stat(v) for k, v in times.items()},
                   set16_over_list16=round(med["set16"] / med["list16"], 2),
                   fetch_over_set1000=round(med["fetch"] / med["set1000"], 1), fetch_over_set10000=round(med["fetch"] / med["set10000"], 1),
                   set16_vs_list16="faster" if max(times["set16"]) < min(times["list16"]) else "slower" if min(times["set16"]) > max(times["list16"]) else "not shown",
                   faster_than_fetch="shown" if min(times["fetch"]) > max(times["set1000"] + times["set10000"]) else "not shown")
        for ps, _ in sets.values():
            ps.free()
        sc.free(d); sc.close()
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
