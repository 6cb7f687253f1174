"""sx_result_order_device against its yardsticks: BASELINE config 5's Missions on GIB GiB of background, as tools/gpu_seen_counts.py.
usage: tools/gpu_order.py [--reps N] [--out FILE] [--host-sort] [--no-pathological] [GIB ...]      (default: 4; profiler off)
After a warm-up of every path, N times each (default 3), the host clock around calls that end synchronised:
  string_all        by string, every finding
  string_first      by string, any = SX_DISTINCT_FIRST: sort -u (the distinct call that made the labels is timed apart: distinct)
  count_top20       by the distinct words' count, descending, any = FIRST, limit = 20: uniq -c | sort -rn | head -20
  everything        sx_result_select_labels_device(words) with no mask: the whole part gathered — result_gather_kernel's time on it is
                    the yardstick of DESIGN.md §7 item 7
  download          every segment's records and strings to pinned host memory: what the caller does today before it can sort
  host_sorted       (--host-sort, once) Python's sorted() over the downloaded strings: the rest of today's alternative
  pathological      once, on a context of its own: 10 000 lines that share a 4 000-byte prefix (ascii and utf-8, -q 4100: 20 000 findings), by string
Checked once, outside the timed region: the ordered strings are sorted and are the source's (how often every byte value and every length
occurs; --host-sort: byte for byte against sorted()); string_first holds info.distinct findings; count_top20's counts
descend.  One JSON line per size (stdout, and appended to FILE) with every call's sx_order_info.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` with `--reps 1 --no-pathological 4`, a run of its own."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import stringsext_amd as sx
from gpu_select import C5, F16, SEED, stat

F32 = np.dtype({"names": ["position", "str_off", "str_len"], "formats": ["<u8", "<u4", "<u4"], "offsets": [0, 8, 12], "itemsize": 32})
FIRST = sx.SX_DISTINCT_FIRST


def timed(call):
    t0 = time.perf_counter()
    x = call()
    return (time.perf_counter() - t0) * 1e3, x


def note(what):
    print("[gpu_order] " + what, file=sys.stderr, flush=True)


PINNED = {"hip": None, "pinned": True}


def pinned(n):
    """n bytes of pinned host memory as a numpy array (hipHostMalloc; kept for the life of the process).  Where the runtime's library
    cannot be had by name the memory is pageable, and the row says so"""
    import ctypes as C
    n = max(n, 1)
    if PINNED["hip"] is None:
        for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
            try:
                PINNED["hip"] = C.CDLL(name)
                break
            except OSError:
                PINNED["hip"] = False
    p = C.c_void_p()
    if PINNED["hip"] and PINNED["hip"].hipHostMalloc(C.byref(p), C.c_size_t(n), C.c_uint(0)) == 0 and p.value:
        return np.ctypeslib.as_array((C.c_uint8 * n).from_address(p.value))
    PINNED["pinned"] = False
    return np.empty(n, dtype=np.uint8)


def download(sc, res, bufs=None):
    """every segment's records and strings into pinned host memory; returns [(records, arena, packed)] as numpy views"""
    import ctypes as C
    out = []
    for k, (fp, n, ap, alen, packed, _) in enumerate(res.device_segments()):
        rb, ab = n * (16 if packed else 32), alen
        if bufs is not None and k >= len(bufs):
            bufs.append((pinned(rb), pinned(ab)))
        r, a = bufs[k] if bufs is not None else (pinned(rb), pinned(ab))
        assert len(r) >= rb and len(a) >= ab
        sc._chk(sx.lib().sx_device_download(sc.h, C.c_void_p(r.ctypes.data), C.c_void_p(fp), rb))
        if ab:
            sc._chk(sx.lib().sx_device_download(sc.h, C.c_void_p(a.ctypes.data), C.c_void_p(ap), ab))
        out.append((r[:rb].view(F16 if packed else F32), a[:ab], packed))
    return out


def strings_of(segs):
    out = []
    for recs, arena, _ in segs:
        b = arena.tobytes()
        out += [b[o:o + n] for o, n in zip(recs["str_off"].tolist(), recs["str_len"].tolist())]
    return out


def digest(segs):
    """what does not depend on the order of the findings: their number, their bytes, how often every byte value and every length occurs"""
    n, total, by_byte, by_len = 0, 0, np.zeros(256, dtype=np.int64), np.zeros(1 << 16, dtype=np.int64)
    for recs, arena, _ in segs:
        ln = recs["str_len"].astype(np.int64)
        by_byte += np.bincount(arena, minlength=256)
        by_len += np.bincount(np.minimum(ln, (1 << 16) - 1), minlength=1 << 16)
        n += len(ln); total += int(ln.sum())
    return n, total, by_byte.tolist(), by_len.tolist()


def is_sorted(segs):
    (recs, arena, _), = segs
    n = len(recs)
    at = np.arange(0, n - 1, max(1, n // 2_000_000))          # (every pair below two million findings; a sample of neighbours above)
    b = arena.tobytes()
    o0, n0, o1, n1 = (x.tolist() for x in (recs["str_off"][at], recs["str_len"][at], recs["str_off"][at + 1], recs["str_len"][at + 1]))
    return all(b[a:a + x] <= b[c:c + y] for a, x, c, y in zip(o0, n0, o1, n1))


def pathological():
    lines, prefix_bytes = 10_000, 4_000
    ms = sx.missions_from_flags(encodings=["ascii", "utf-8"], chars_min="4", output_line_len="4100")      # (two Missions: the merged result stays in HBM)
    stem = bytes(97 + (i * 7 + i // 26) % 26 for i in range(prefix_bytes))
    data = b"\n".join(stem + b"%05d" % (i * 7919 % lines) for i in range(lines)) + b"\n"
    sc = sx.Scanner(ms, device=0, result_on_device=True)
    res = sc.scan(data, file_id=1)
    assert len(res) == 2 * lines and all(s[0] is not None for s in res.device_segments()), len(res)
    res.order_device().free()
    dt, o = timed(res.order_device)
    info = o.order_info
    got = strings_of(download(sc, o))
    assert got == sorted(data.split(b"\n")[:-1] * 2)
    o.free(); res.free(); sc.close()
    return dict(tool="gpu_order", pathological=dict(lines=lines, findings=2 * lines, prefix_bytes=prefix_bytes, ms=round(dt, 3), info=info))


def main():
    args, reps, out, host_sort, hard = sys.argv[1:], 3, None, False, True
    while args and args[0].startswith("--"):
        if args[0] == "--reps":
            reps, args = int(args[1]), args[2:]
        elif args[0] == "--out":
            out, args = args[1], args[2:]
        elif args[0] == "--host-sort":
            host_sort, args = True, args[1:]
        elif args[0] == "--no-pathological":
            hard, args = False, args[1:]
        else:
            sys.exit(__doc__)
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
        findings, str_bytes, n_segs = len(res), sum(s[3] for s in segs), len(segs)
        note("%d findings, %d bytes of strings in %d segments" % (findings, str_bytes, n_segs))
        # warm-up of all paths, and the checks
        lab = res.distinct_device()
        bufs = []
        src = download(sc, res, bufs)
        want = digest(src)
        assert want[:2] == (findings, str_bytes)
        host_ms = None
        o = res.order_device()
        got = download(sc, o)
        assert digest(got) == want and is_sorted(got) and o.order_info["findings"] == o.order_info["kept"] == findings, o.order_info
        note("ordered and checked: %r" % (o.order_info,))
        if host_sort:
            t0 = time.perf_counter()
            strs = strings_of(src)
            t1 = time.perf_counter()
            strs.sort()
            note("sorted on the host")
            host_ms = dict(strings_ms=round((t1 - t0) * 1e3, 1), sorted_ms=round((time.perf_counter() - t1) * 1e3, 1))
            assert strings_of(got) == strs
            del strs
        del got
        infos = dict(string_all=o.order_info)
        o.free()
        o = res.order_device(labels=lab, any=FIRST)
        got = download(sc, o)
        assert len(o) == lab.info["distinct"] and is_sorted(got) and o.order_info["tied"] == 0
        infos["string_first"] = o.order_info
        o.free()
        o = res.order_device("field", lab, shift=32, bits=32, descending=True, any=FIRST, limit=20)
        infos["count_top20"] = o.order_info
        top = o.findings()
        assert len(top) == min(20, lab.info["distinct"])
        o.free()
        res.select_device(lab).free()
        names = ("distinct", "string_all", "string_first", "count_top20", "everything", "download")
        times = {k: [] for k in names}
        note("warm")
        for _ in range(reps):
            lab.free()
            dt, lab = timed(res.distinct_device)
            times["distinct"].append(dt)
            for name, call in (("string_all", res.order_device), ("string_first", lambda: res.order_device(labels=lab, any=FIRST)),
                               ("count_top20", lambda: res.order_device("field", lab, shift=32, bits=32, descending=True, any=FIRST, limit=20)),
                               ("everything", lambda: res.select_device(lab))):
                dt, x = timed(call)
                times[name].append(dt)
                x.free()
            times["download"].append(timed(lambda: download(sc, res, bufs))[0])
        row = dict(tool="gpu_order", gib=gib, missions="c5", reps=reps, findings=findings, segments=n_segs, string_bytes=str_bytes, distinct=lab.info,
                   info=infos, top=[f["s"][:40] for f in top[:3]], host=host_ms, pinned=PINNED["pinned"], **{k + "_ms": stat(v) for k, v in times.items()})
        lab.free(); res.free()
        sc.free(d); sc.close()
        emit(json.dumps(row), out)
    if hard:
        emit(json.dumps(pathological()), out)


def emit(line, out):
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
