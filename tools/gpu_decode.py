"""The decoding of a device-resident result's base64 strings (sx_result_decode_device) against its yardsticks: BASELINE config 5's
Missions on GIB GiB of background, as tools/gpu_fold.py.
usage: tools/gpu_decode.py [--reps N] [--out FILE] [GIB ...]      (default: 4; profiler off)
After a warm-up of every path, alternating, N times each (default 5), the host clock around calls that end synchronised:
  base64      one sx_result_decode_device call with SX_DECODE_BASE64: a new result and the words, with sx_decode_info
  base64_u16  the same with SX_DECODE_UTF16LE
  fold        one sx_result_fold_device call on the same result: the operation of the same shape
  everything  sx_result_select_device with a pattern that cannot occur, inverted: the whole part selected and gathered —
              result_gather_kernel's time on it is the yardstick of DESIGN.md §7 item 7
Checked once, outside the timed region: the strings and the words of the first 200 000 findings of segment 0 are those of the rule in
Python (tests/decode_plant.py: the conditions of include/stringsext_amd.h, then base64 and codecs), every other byte of their records
is the source's, and sx_decode_info's bytes are the segments' bytes.  One JSON line per size (stdout, and appended to FILE).
Kernel times: run this under `rocprofv3 --kernel-trace --stats` with `--reps 2 4`, a run of its own: per call and segment the launches
are decode_measure_kernel, rocprim's scan and decode_place_kernel."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import stringsext_amd as sx
from gpu_select import C5, F16, SEED, stat
import decode_plant as dp      # (tests/: gpu_select has put it on the path)

CANNOT_OCCUR = b"\x02\x02"
CHECKED = 200_000


def check(sc, res, d, flags):
    """the first CHECKED findings of segment 0 of `d`, decoded from `res`, against the rule; returns how many of them decode"""
    (fp, n0, ap, _, packed, _), (dfp, _, dap, _, _, _) = res.device_segments()[0], d.device_segments()[0]
    assert packed
    k = min(n0, CHECKED)
    recs, drecs = (np.frombuffer(sc.download(C.c_void_p(p), k * 16), dtype=F16) for p in (fp, dfp))
    arena, darena = (sc.download(C.c_void_p(p), int(r[-1]["str_off"]) + int(r[-1]["str_len"])) for p, r in ((ap, recs), (dap, drecs)))
    words = np.frombuffer(sc.download(C.c_void_p(d.decode_words.device_segments()[0][0]), k * 8), dtype="<u8")
    decoded = 0
    for r, f, w in zip(recs, drecs, words.tolist()):
        s = arena[int(r["str_off"]):int(r["str_off"]) + int(r["str_len"])]
        g = darena[int(f["str_off"]):int(f["str_off"]) + int(f["str_len"])]
        want = dp.decode(dp.BASE64, flags, s)
        assert (g, w) == want and (r["position"], r["flags"], r["mission_id"]) == (f["position"], f["flags"], f["mission_id"]), ("the rule decodes otherwise", s, g, w, want)
        decoded += w & 1
    return k, decoded


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
        buf = sc.alloc(total)
        sc.fill_background(buf, 0, total, SEED)
        sc.reset()
        res = sc.scan_device(buf, total, file_id=1)
        segs = res.device_segments()
        assert all(s[0] is not None for s in segs)
        findings, str_bytes, n_segs = len(res), sum(s[3] for s in segs), len(segs)

        def timed(call):
            t0 = time.perf_counter()
            got = call()
            return (time.perf_counter() - t0) * 1e3, got

        def free(d):
            if d.decode_words is not None:
                d.decode_words.free()
            d.free()

        calls = {"base64": lambda: res.decode_device("base64"), "base64_u16": lambda: res.decode_device("base64", utf16le=True),
                 "fold": res.fold_device, "everything": lambda: res.select_device(CANNOT_OCCUR, invert=True)}
        # warm-up of all paths, and the checks
        infos, checked = {}, {}
        for name, flags in (("base64", 0), ("base64_u16", dp.UTF16LE)):
            d = calls[name]()
            info = infos[name] = d.decode_info
            dsegs = d.device_segments()
            assert [(s[1], s[4]) for s in dsegs] == [(s[1], s[4]) for s in segs] and info["findings"] == findings, (info, dsegs)
            assert info["bytes_in"] == str_bytes and info["bytes_out"] == sum(s[3] for s in dsegs), (info, str_bytes)
            checked[name] = check(sc, res, d, flags)
            free(d)
        for name in ("fold", "everything"):
            d = calls[name]()
            assert len(d) == findings
            d.free()
        times = {k: [] for k in calls}
        for _ in range(reps):
            for name, call in calls.items():
                dt, d = timed(call)
                times[name].append(dt)
                free(d)
        res.free()
        row = dict(tool="gpu_decode", gib=gib, missions="c5", reps=reps, findings=findings, segments=n_segs, string_bytes=str_bytes, info=infos,
                   checked={k: dict(findings=v[0], decoded=int(v[1])) for k, v in checked.items()}, **{k + "_ms": stat(v) for k, v in times.items()})
        sc.free(buf); sc.close()
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
