"""The approximate matches of a device-resident result (sx_fuzzy_set_create / sx_result_fuzzy_device) against their yardsticks:
BASELINE config 5's Missions on GIB GiB of background, as tools/gpu_label.py.
usage: tools/gpu_fuzzy.py [--reps N] [--out FILE] [GIB ...]      (default: 4; profiler off)
After a warm-up of every path, alternating, N times each (default 5), the host clock around calls that end synchronised:
  fuzzy P k   one sx_result_fuzzy_device call with the first P of KEYWORDS (P = 1, 8, 64) at k errors each (k = 1, 2); keywords of at
              most 32 bytes, so the 32-bit kernel; `fuzzy 8 2 wide` is the eight with one keyword of 40 bytes beside them: the 64-bit kernel
  label6      the same result's sx_result_label_device call with tools/gpu_label.py's six patterns
  download    what a host would need before it could compute anything: every segment's strings through sx_device_download
Checked once, outside the timed region: the words of the first 2 000 findings of segment 0 are tests/fuzzy_plant.py's — Sellers' table
in Python — and sx_fuzzy_bytes' for every set; the set's count per pattern is the number of findings with that bit.  One JSON line per
size (stdout, and appended to FILE) with the sets' info.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` with `--reps 2 4`, a run of its own: per timed repetition the launches
are fuzzy_match_kernel once per set and segment and label_match_kernel once per segment."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import stringsext_amd as sx
from gpu_select import C5, F16, SEED, stat
from gpu_select_regex import SHAPES

import fuzzy_plant as fz      # (tests/: gpu_select has put it on the path)

KEYWORDS = (fz.WORDS + [b"passwd", b"authorized_keys", b"id_rsa", b"Authorization: Bearer", b"api_key", b"AKIA", b"-----BEGIN", b"wallet.dat", b"mimikatz",
                        b"powershell -enc", b"cmd.exe /c", b"/bin/sh", b"LD_PRELOAD", b"HKEY_LOCAL_MACHINE", b"CurrentVersion\\Run", b"schtasks"]
            + [b"indicator-%02d.example" % i for i in range(36)])
WIDE = b"the quick brown fox jumps over the lazy dog"[:40]
SETS = [("fuzzy %d %d" % (p, k), KEYWORDS[:p], k) for p in (1, 8, 64) for k in (1, 2)] + [("fuzzy 8 2 wide", KEYWORDS[:8] + [WIDE], 2)]
assert len(KEYWORDS) == 64 and all(2 < len(w) <= 32 for w in KEYWORDS)


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
            got = call()
            return (time.perf_counter() - t0) * 1e3, got

        def download(res):
            return sum(len(sc.download(C.c_void_p(s[2]), s[3])) for s in res.device_segments())

        sets = {name: sc.fuzzy_set(pats, k) for name, pats, k in SETS}
        ls = sc.label_set(SHAPES)
        # warm-up of all paths, and the checks
        res = scan()
        segs = res.device_segments()
        findings, str_bytes, n_segs = len(res), sum(s[3] for s in segs), len(segs)
        fp, n0, ap, _, packed, _ = segs[0]
        assert packed
        k0 = min(n0, 2000)
        recs = np.frombuffer(sc.download(C.c_void_p(fp), k0 * 16), dtype=F16)
        arena = sc.download(C.c_void_p(ap), int(recs[-1]["str_off"]) + int(recs[-1]["str_len"]))
        strs = [arena[int(r["str_off"]):int(r["str_off"]) + int(r["str_len"])] for r in recs]
        counted = {}
        for name, pats, k in SETS:
            lab = res.fuzzy_device(sets[name])
            words = [np.frombuffer(sc.download(C.c_void_p(p), n * 8), dtype="<u8") for p, n in lab.device_segments()]
            assert np.array_equal(words[0][:k0], fz.words(pats, k, strs)), ("Sellers' table says otherwise", name)
            assert all(sx.fuzzy(pats, k, s) == int(w) for s, w in zip(strs[:200], words[0])), ("sx_fuzzy_bytes says otherwise", name)
            every = np.concatenate(words)
            counted[name] = sets[name].read()[0]
            assert counted[name] == [int(((every >> np.uint64(p)) & np.uint64(1)).sum()) for p in range(len(pats))], ("the counters and the words differ", name)
            sets[name].reset()
            lab.free()
        res.label_device(ls).free()
        assert download(res) == str_bytes
        res.free()
        times = {name: [] for name in list(sets) + ["label6", "download"]}
        for _ in range(reps):
            res = scan()
            for name in sets:
                dt, lab = timed(lambda: res.fuzzy_device(sets[name]))
                times[name].append(dt)
                lab.free()
            dt, lab = timed(lambda: res.label_device(ls))
            times["label6"].append(dt)
            lab.free()
            times["download"].append(timed(lambda: download(res))[0])
            res.free()
        row = dict(tool="gpu_fuzzy", gib=gib, missions="c5", reps=reps, findings=findings, segments=n_segs, string_bytes=str_bytes,
                   matched={name: sum(v) for name, v in counted.items()},
                   info={name: {f: getattr(s.info, f) for f, _ in sx.FuzzySetInfo._fields_} for name, s in sets.items()},
                   **{name.replace(" ", "_") + "_ms": stat(v) for name, v in times.items()})
        for x in list(sets.values()) + [ls]:
            x.free()
        sc.free(d); sc.close()
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
