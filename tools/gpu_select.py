"""The substring selection on the device against fetching the result: BASELINE config 5's Missions on GIB GiB of background.
usage: tools/gpu_select.py [--reps N] [--out FILE] [GIB ...]      (default: 4 16; profiler off)
After a warm-up of all three, alternating, N times each (default 5):
  select1   sx_result_select_device with ONE 4-byte pattern on a result that lies in HBM (host clock around the call; it ends synchronised)
  select16  the same with 16 patterns of 4 bytes
  fetch     a fresh scan with SX_OPT_RESULT_ON_DEVICE, then every segment fetched to the host (Result.packed_segments(), which
            copies each segment over PCIe): the only way to the selection's INPUT without the device call, and so the floor under
            any search on the host, which has yet to begin then.  (The scan is not timed.)
The patterns are the middle four bytes of strings of the result's first segment (16 of them, spread over the segment; the first one
alone for select1).  The number of selected findings is checked against a search over the fetched segments once, outside the
timed region.  One JSON line per size (stdout, and appended to FILE)."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np

import stringsext_amd as sx

SEED = 0x5EED5EED5EED5EED   # BASELINE.md §3 (tests/test_gpu_baseline_configs.py)
C5 = dict(encodings=["utf-8,,,African", "utf-16le,,,African", "utf-16be,,,African", "big5,,,Cjk", "euc-jp,,,Asian", "koi8-r,,,Cyrillic"], chars_min="10")
PEAK = 8e12                 # HBM3E, bytes per second
F16 = np.dtype({"names": ["position", "str_off", "str_len", "flags", "mission_id"], "formats": ["<u8", "<u4", "<u2", "u1", "u1"],
                "offsets": [0, 8, 12, 14, 15], "itemsize": 16})


def stat(v):
    s = sorted(v)
    return dict(median=round(s[len(s) // 2], 3), min=round(s[0], 3), max=round(s[-1], 3))


def count_on_host(segments, patterns):
    """findings whose string holds one of the patterns: every occurrence in the arena, kept if it ends inside the record it begins in"""
    total = 0
    for packed, recs, n, arena, _ in segments:
        assert packed
        r = np.frombuffer(C.string_at(recs, n * 16), dtype=F16)
        off = r["str_off"].astype(np.int64)
        end = off + r["str_len"].astype(np.int64)
        assert np.all(off[1:] == end[:-1])      # back to back, in record order
        hit = np.zeros(n, bool)
        for p in patterns:
            at = arena.find(p)
            while at >= 0:
                i = int(np.searchsorted(off, at, side="right")) - 1
                while end[i] <= at:             # (empty strings share their successor's offset)
                    i += 1
                if at + len(p) <= end[i]:
                    hit[i] = True
                at = arena.find(p, at + 1)
        total += int(hit.sum())
    return total


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

        # the patterns, a warm-up of all paths (the blocks and the pinned pool get their sizes), and the one comparison
        res = scan()
        segs = res.device_segments()
        findings, str_bytes, n_segs = len(res), sum(s[3] for s in segs), len(segs)
        rec_bytes = sum(s[1] * (16 if s[4] else 32) for s in segs)
        fp, n0, ap, alen, packed, _ = segs[0]
        assert packed
        patterns = []
        for k in range(16):
            r = np.frombuffer(sc.download(C.c_void_p(fp + (k * n0 // 16) * 16), 16), dtype=F16)[0]
            o = int(r["str_off"]) + (int(r["str_len"]) - 4) // 2
            patterns.append(sc.download(C.c_void_p(ap + o), 4))
        _, n1 = select(res, patterns[:1])
        _, n16 = select(res, patterns)
        res.select_device(b"\xff" * 4).free()   # (nothing selected: both blocks have been used)
        fetch(res)
        got = res.packed_segments()
        assert count_on_host(got, patterns[:1]) == n1 and count_on_host(got, patterns) == n16, "the device's selection differs from a search on the host"
        res.free()
        one, sixteen, host = [], [], []
        for _ in range(reps):
            res = scan()
            one.append(select(res, patterns[:1])[0])
            sixteen.append(select(res, patterns)[0])
            res.free()
            res = scan()
            host.append(fetch(res))
            res.free()
        sc.free(d); sc.close()
        # what the match kernel moves: every record once (twice: the neighbour's offset, L1), every string byte once, 20 bytes per 64 records
        moved = rec_bytes + str_bytes + findings // 64 * 20
        row = dict(tool="gpu_select", gib=gib, missions="c5", reps=reps, findings=findings, segments=n_segs, string_bytes=str_bytes,
                   record_bytes=rec_bytes, patterns=[p.hex() for p in patterns], selected_1=n1, selected_16=n16,
                   select1_ms=stat(one), select16_ms=stat(sixteen), fetch_ms=stat(host), match_bytes=moved,
                   select1_call_gbps=round(moved / (stat(one)["median"] * 1e-3) / 1e9, 1),
                   select16_call_gbps=round(moved / (stat(sixteen)["median"] * 1e-3) / 1e9, 1),
                   select1_share_of_8tbps=round(moved / (stat(one)["median"] * 1e-3) / PEAK, 4), rate_is="call time, not kernel time",
                   fetch_over_select1=round(stat(host)["median"] / stat(one)["median"], 1),
                   fetch_over_select16=round(stat(host)["median"] / stat(sixteen)["median"], 1),
                   faster="shown" if min(host) > max(max(one), max(sixteen)) else "not shown")
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
