"""Finding::print on the device against the host's: BASELINE config 5's Missions on GIB GiB of background, radix x.
usage: tools/gpu_print.py [--reps N] [--out FILE] [GIB ...]      (default: 4 16; profiler off)
After a warm-up of both, alternating, N times each (default 5):
  device     sx_print_findings_device on a result that lies in HBM (host clock around the call; it ends synchronised)
  device+d2h the same call plus a copy of the text into pinned host memory: the end-to-end figure comparable with ...
  host       a fresh scan with SX_OPT_RESULT_ON_DEVICE, then sx_print_findings on it, which fetches the segments and formats them
             on the host: what a caller without the device call does.  (The scan is not timed.)
Both texts are compared once, outside the timed region.  One JSON line per size (stdout, and appended to FILE)."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import stringsext_amd as sx

SEED = 0x5EED5EED5EED5EED   # BASELINE.md §3 (tests/test_gpu_baseline_configs.py)
C5 = dict(encodings=["utf-8,,,African", "utf-16le,,,African", "utf-16be,,,African", "big5,,,Cjk", "euc-jp,,,Asian", "koi8-r,,,Cyrillic"], chars_min="10")
PEAK = 8e12                 # HBM3E, bytes per second


def stat(v):
    s = sorted(v)
    return dict(median=round(s[len(s) // 2], 3), min=round(s[0], 3), max=round(s[-1], 3))


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
    hip = C.CDLL("libamdhip64.so")
    hip.hipHostMalloc.argtypes, hip.hipHostFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint], [C.c_void_p]
    libc = C.CDLL(None)
    libc.memcmp.argtypes, libc.memcmp.restype = [C.c_void_p, C.c_void_p, C.c_size_t], C.c_int
    L = sx.lib()
    ms = sx.missions_from_flags(**C5)
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

        def host_print(res, keep=False):
            p, n = C.POINTER(C.c_uint8)(), C.c_uint64()
            t0 = time.perf_counter()
            sc._chk(L.sx_print_findings(sc.h, res.h, 1, ord("x"), 0, C.byref(p), C.byref(n)))
            dt = (time.perf_counter() - t0) * 1e3
            if keep:
                return dt, p, n.value
            L.sx_free(p)
            return dt, None, n.value

        # warm-up of both paths (the text block and the pinned pool get their sizes), and the one comparison
        res = scan()
        segs = res.device_segments()
        findings, str_bytes, n_segs = len(res), sum(s[3] for s in segs), len(segs)
        rec_bytes = sum(s[1] * (16 if s[4] else 32) for s in segs)
        p, n = res.printed_device(n_inputs=1, radix="x")
        pin = C.c_void_p()
        assert hip.hipHostMalloc(C.byref(pin), n, 0) == 0
        sc._chk(L.sx_device_download(sc.h, pin, C.c_void_p(p), n))
        _, hp, hn = host_print(res, keep=True)
        assert hn == n and libc.memcmp(hp, pin, n) == 0, "the device's text differs from sx_print_findings'"
        L.sx_free(hp); res.free()
        dev, e2e, host = [], [], []
        for _ in range(reps):
            res = scan()
            t0 = time.perf_counter()
            p, n2 = res.printed_device(n_inputs=1, radix="x")
            dev.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            p, n2 = res.printed_device(n_inputs=1, radix="x")
            sc._chk(L.sx_device_download(sc.h, pin, C.c_void_p(p), n2))
            e2e.append((time.perf_counter() - t0) * 1e3)
            assert n2 == n
            res.free()
            res = scan()
            host.append(host_print(res)[0])
            res.free()
        hip.hipHostFree(pin)
        sc.free(d); sc.close()
        # what the two kernels move: every record twice (length pass, write pass), every string byte once, every text byte once,
        # the wavefronts' sums and offsets (8 bytes per 64 records, written and read twice)
        moved = 2 * rec_bytes + str_bytes + n + findings // 64 * 32
        spread = max(host) - min(host)
        gain = min(host) - max(e2e)
        row = dict(tool="gpu_print", gib=gib, missions="c5", radix="x", reps=reps, findings=findings, segments=n_segs, text_bytes=n,
                   string_bytes=str_bytes, record_bytes=rec_bytes, device_ms=stat(dev), device_plus_d2h_ms=stat(e2e), host_ms=stat(host),
                   kernel_bytes=moved, call_gbps=round(moved / (stat(dev)["median"] * 1e-3) / 1e9, 1),
                   call_share_of_8tbps=round(moved / (stat(dev)["median"] * 1e-3) / PEAK, 4), rate_is="call time, not kernel time",
                   host_over_device_plus_d2h=round(stat(host)["median"] / stat(e2e)["median"], 1),
                   faster="shown" if gain > spread else "not shown", host_spread_ms=round(spread, 3), worst_case_gain_ms=round(gain, 3))
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
