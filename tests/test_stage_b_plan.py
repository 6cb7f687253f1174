"""The pure decisions of stage B's host drivers (stringsext_amd/csrc/sx_stage_b_plan.hpp: where the exit state is replayed from,
which slab cuts stand, how device_merge sizes its parts, a slab's output layout, the size of pass 1's cache arena) compiled as plain
host C++ (tests/native/stage_b_plan_host.cpp) against Python transcriptions of the expressions the drivers held inline before the
header existed — 10 000 seeded random inputs per function and the named edges.  The same cases go through a stand-alone program built
with the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
sys.path.insert(0, NATIVE)
import build_harness  # noqa: E402

M64 = (1 << 64) - 1
BUF = 4096                       # kInputBufLen
REC, REC16 = 32, 16              # sizeof(sx_finding), sizeof(sx_finding16)
N_RANDOM = 10000


# ---- the drivers' expressions, as they stood (u64 arithmetic: wraps are kept)
def win_start(p, W):
    s0 = p // BUF * BUF
    return s0 + (p - s0) // W * W


def exit_from(length, W, lo0, E, last_start, last_is_entry):
    tail = length - 1 if length else 0
    ts = win_start(tail, W)
    for _ in range(3):
        if ts > 0:
            ts = win_start(ts - 1, W)
    frm = lo0 if last_is_entry else (last_start if E > ts else ts)
    return [max(frm, lo0)]


def slab_cuts(K, n, job_hi, *h):
    h_idx, h_hi = h[:K - 1], h[K - 1:2 * (K - 1)]
    idx, his = [0], [0]
    for j in range(1, K):
        if h_idx[j - 1] > idx[-1] and h_idx[j - 1] < n and h_hi[j - 1] < job_hi:
            idx.append(h_idx[j - 1]); his.append(h_hi[j - 1])
    return [len(idx)] + idx + his


def merge_first_k(nbytes, total, part_mib, part_findings_sw):
    part_bytes, part_findings = 2048 << 20, 96 << 20
    if part_mib:
        part_bytes = (part_mib << 20) & M64
    if part_findings_sw:
        part_findings = part_findings_sw
    if part_bytes > (3584 << 20):
        part_bytes = 3584 << 20
    K = max(1, max((nbytes + part_bytes - 1) // part_bytes, (total + part_findings - 1) // part_findings))
    return [part_bytes, part_findings, K]


def merge_clamp_k(K, n_slices):
    if K > n_slices:
        K = max(1, n_slices)
    return [K]


def merge_parts(nm, K, part_findings, n_slices, *rows):
    idx = [rows[k * 2 * (K + 1):k * 2 * (K + 1) + K + 1] for k in range(nm)]
    off = [rows[k * 2 * (K + 1) + K + 1:(k + 1) * 2 * (K + 1)] for k in range(nm)]
    parts, fits = [], True
    for j in range(K):
        pb = sum(off[k][j + 1] - off[k][j] for k in range(nm)) & M64
        pf = sum(idx[k][j + 1] - idx[k][j] for k in range(nm)) & M64
        parts += [pf, pb]
        fits = fits and pb <= 0xFFFFFFF0 and (pf <= 2 * part_findings or K >= n_slices)
    return [int(fits)] + parts


def part_room(pf, rec, pb):
    return [(pf * rec + pb + 255) & ~255 & M64]


def slab_out(nfh, nf, nbh, nb, rec):
    return [nfh * rec, (nfh + nf) * rec, (nfh + nf) * rec + nbh, (nfh + nf) * rec + nbh + nb, nfh + nf, nbh + nb, int(nb + nbh <= 0xFFFFFFFF)]


def cache_arena(n, free_plus_held, cache_mib):
    cache_mib = cache_mib - (1 << 64) if cache_mib >> 63 else cache_mib      # (an int64 in the switches' table; -1: unset)
    budget = 8192 << 20
    asks = n * 160 > budget
    if asks and free_plus_held:
        budget = max(budget, min(40960 << 20, free_plus_held // 3))
    if cache_mib >= 0:
        budget = cache_mib << 20
    return [int(asks), max(4096, min(budget, n * 1024))]


RULES = {"win_start": lambda p, W: [win_start(p, W)], "exit_from": exit_from, "slab_cuts": slab_cuts, "merge_first_k": merge_first_k, "merge_clamp_k": merge_clamp_k,
         "merge_parts": merge_parts, "part_room": part_room, "slab_out": slab_out, "cache_arena": cache_arena}


# ---- cases: (function, arguments)
def sizes(rng):
    """a length, with the small ones and those around the buffer grid well represented"""
    return rng.choice((rng.randrange(0, 40), rng.randrange(0, 3 * BUF), rng.randrange(0, 1 << 20), rng.randrange(0, 1 << 34),
                       BUF * rng.randrange(0, 1 << 20) + rng.choice((-1, 0, 1)) % BUF))


def windows(rng):
    return rng.choice((32, 64, 128, 256, 512, 1024, 4096, rng.randrange(1, 4097)))


def monotone(rng, K, end):
    cuts = sorted(rng.randrange(0, end + 1) for _ in range(K - 1))
    return [0] + cuts + [end]


def merge_parts_case(rng, nm, K, part_findings=None, n_slices=None, big=False, empty_part=False):
    rows = []
    for _ in range(nm):
        idx = monotone(rng, K, rng.randrange(0, 1 << (28 if big else 16)))
        off = monotone(rng, K, rng.randrange(0, 1 << (34 if big else 20)))
        if empty_part and K > 1:
            idx[2 if K > 2 else 1] = idx[1]                                   # part 1 holds no finding of this Mission
        rows += idx + off
    return ("merge_parts", [nm, K, part_findings or rng.choice((1024, 1 << 20, 96 << 20)), n_slices or rng.choice((1, K, K + 1, 1 << 20))] + rows)


def named_cases():
    c = []
    # exit state: len == 0, len < W, the walk back reaching 0, last_is_entry, from < lo0, E on both sides of ts
    c += [("exit_from", [0, 128, 0, 0, 0, 0]), ("exit_from", [0, 128, 0, 5, 3, 1]), ("exit_from", [100, 128, 0, 50, 10, 0]),
          ("exit_from", [100, 128, 7, 0, 0, 0]), ("exit_from", [4 * 128, 128, 0, 1, 0, 0]), ("exit_from", [3 * 128 + 1, 128, 0, 1, 0, 0]),
          ("exit_from", [1 << 20, 128, 4096, 1 << 19, 1 << 18, 1]), ("exit_from", [1 << 20, 128, 1 << 19, 1 << 20, 100, 0]),
          ("exit_from", [1 << 20, 128, (1 << 20) - 64, 0, 0, 0])]
    ts = win_start(win_start(win_start(win_start((1 << 20) - 1, 128) - 1, 128) - 1, 128) - 1, 128)
    c += [("exit_from", [1 << 20, 128, 0, ts, 4096, 0]), ("exit_from", [1 << 20, 128, 0, ts + 1, 4096, 0]), ("exit_from", [1 << 20, 128, 0, ts - 1, 4096, 0])]
    assert exit_from(1 << 20, 128, 0, ts, 4096, 0) == [ts] and exit_from(1 << 20, 128, 0, ts + 1, 4096, 0) == [4096]
    assert exit_from(4 * 128, 128, 0, 1, 0, 0) == [0] and exit_from(1 << 20, 128, 1 << 19, 1 << 20, 100, 0) == [1 << 19]
    # windows that do not divide the buffer: the last window of a buffer is short
    c += [("win_start", [4095, 100]), ("win_start", [4096, 100]), ("win_start", [4000, 100]), ("win_start", [0, 1]), ("win_start", [8191, 4096])]
    # slab cuts: a cut equal to the one before, a cut equal to n, hi >= job.hi, and all three standing
    c += [("slab_cuts", [3, 100, 1 << 20, 40, 40, 4096, 8192]), ("slab_cuts", [3, 100, 1 << 20, 40, 100, 4096, 8192]),
          ("slab_cuts", [3, 100, 8192, 40, 70, 4096, 8192]), ("slab_cuts", [4, 100, 1 << 20, 20, 50, 80, 4096, 8192, 12288]),
          ("slab_cuts", [2, 100, 1 << 20, 0, 0]), ("slab_cuts", [1, 100, 1 << 20])]
    assert slab_cuts(3, 100, 1 << 20, 40, 40, 4096, 8192) == [2, 0, 40, 0, 4096] and slab_cuts(3, 100, 1 << 20, 40, 100, 4096, 8192) == [2, 0, 40, 0, 4096]
    assert slab_cuts(3, 100, 8192, 40, 70, 4096, 8192) == [2, 0, 40, 0, 4096]
    # the merger: the 3584 MiB clamp, the switches, K from either bound
    c += [("merge_first_k", [0, 0, 0, 0]), ("merge_first_k", [(2048 << 20) + 1, 5, 0, 0]), ("merge_first_k", [1 << 40, 5, 4000, 0]),
          ("merge_first_k", [1 << 40, 5, 3584, 0]), ("merge_first_k", [5, (96 << 20) * 3 + 1, 0, 0]), ("merge_first_k", [1 << 30, 1 << 30, 1, 1024])]
    assert merge_first_k(1 << 40, 5, 4000, 0)[0] == 3584 << 20 and merge_first_k((2048 << 20) + 1, 5, 0, 0)[2] == 2
    rng = random.Random(77)
    # K > n_slices: a slice per part, one part for an empty buffer; K == n_slices lifts the bound on findings
    c += [("merge_clamp_k", [5, 4]), ("merge_clamp_k", [4, 4]), ("merge_clamp_k", [3, 4]), ("merge_clamp_k", [1, 0]), ("merge_clamp_k", [7, 0]), ("merge_clamp_k", [1 << 40, 1])]
    assert merge_clamp_k(5, 4) == [4] and merge_clamp_k(7, 0) == [1]
    c += [merge_parts_case(rng, 3, 4, part_findings=1024, n_slices=4, big=True), merge_parts_case(rng, 3, 4, part_findings=1024, n_slices=5, big=True),
          merge_parts_case(rng, 2, 3, empty_part=True), merge_parts_case(rng, 1, 1), merge_parts_case(rng, 4, 1, big=True)]
    # a part with no finding at all (pf == 0)
    c += [("merge_parts", [2, 3, 1024, 100, 0, 10, 10, 30, 0, 100, 100, 300, 0, 7, 7, 9, 0, 50, 50, 90])]
    assert merge_parts(2, 3, 1024, 100, 0, 10, 10, 30, 0, 100, 100, 300, 0, 7, 7, 9, 0, 50, 50, 90)[3:5] == [0, 0]
    # a fit check that fails once and passes after doubling: 10 GiB of strings in two parts, then in four
    two = ("merge_parts", [1, 2, 96 << 20, 1 << 20, 0, 1000, 2000, 0, 5 << 30, 10 << 30])
    four = ("merge_parts", [1, 4, 96 << 20, 1 << 20, 0, 500, 1000, 1500, 2000, 0, 5 << 29, 5 << 30, 15 << 29, 10 << 30])
    assert merge_parts(*two[1])[0] == 0 and merge_parts(*four[1])[0] == 1
    c += [two, four]
    c += [("part_room", [0, REC, 0]), ("part_room", [1, REC16, 240]), ("part_room", [8, REC, 0]), ("part_room", [8, REC, 1])]
    # a slab's output: no entry part, packed records, the 4 GiB edge
    c += [("slab_out", [0, 10, 0, 100, REC]), ("slab_out", [3, 10, 40, 100, REC16]), ("slab_out", [0, 0, 0, 0, REC]), ("slab_out", [2, 0, 9, 0, REC16]),
          ("slab_out", [1, 1, 1, 0xFFFFFFFE, REC]), ("slab_out", [1, 1, 1, 0xFFFFFFFF, REC])]
    assert slab_out(1, 1, 1, 0xFFFFFFFE, REC)[6] == 1 and slab_out(1, 1, 1, 0xFFFFFFFF, REC)[6] == 0
    # the cache arena: the floor, 1 KiB per run, the 8 GiB budget, a flood with and without the free memory known, the override
    flood = (8192 << 20) // 160 + 1
    c += [("cache_arena", [0, 0, M64]), ("cache_arena", [3, 0, M64]), ("cache_arena", [1 << 20, 0, M64]), ("cache_arena", [1 << 24, 0, M64]),
          ("cache_arena", [flood - 1, 200 << 30, M64]), ("cache_arena", [flood, 200 << 30, M64]), ("cache_arena", [flood, 0, M64]),
          ("cache_arena", [flood, 30 << 30, M64]), ("cache_arena", [flood, 20 << 30, M64]), ("cache_arena", [1 << 20, 0, 0]), ("cache_arena", [1 << 20, 0, 64]),
          ("cache_arena", [flood, 200 << 30, 64])]
    assert cache_arena(flood, 200 << 30, M64) == [1, 40960 << 20] and cache_arena(flood, 30 << 30, M64) == [1, 10 << 30] and cache_arena(1 << 20, 0, 0) == [0, 4096]
    return c


def random_cases():
    rng = random.Random(20260)
    c = []
    for _ in range(N_RANDOM):
        c.append(("win_start", [sizes(rng), windows(rng)]))
        length, W = sizes(rng), windows(rng)
        at = lambda: rng.choice((0, rng.randrange(0, length + 1), sizes(rng)))   # noqa: E731
        c.append(("exit_from", [length, W, at(), at(), at(), rng.randrange(2)]))
        K, n = rng.randrange(1, 9), rng.randrange(0, 200)
        cuts = [rng.choice((0, n, rng.randrange(0, n + 2))) for _ in range(K - 1)]
        if rng.randrange(2):
            cuts.sort()
        c.append(("slab_cuts", [K, n, rng.choice((0, 1 << 16, 1 << 30))] + cuts + [rng.randrange(0, 1 << 17) for _ in range(K - 1)]))
        c.append(("merge_first_k", [sizes(rng) << rng.randrange(0, 8), sizes(rng), rng.choice((0, 0, 1, 64, 3584, 3585, 1 << 20)), rng.choice((0, 0, 1024, 1 << 30))]))
        c.append(("merge_clamp_k", [rng.randrange(0, 20), rng.randrange(0, 20)]))
        c.append(merge_parts_case(rng, rng.randrange(1, 5), rng.randrange(1, 7), big=rng.randrange(4) == 0, empty_part=rng.randrange(4) == 0))
        c.append(("part_room", [sizes(rng), rng.choice((REC, REC16)), sizes(rng)]))
        c.append(("slab_out", [rng.choice((0, 0, rng.randrange(0, 100))), sizes(rng), rng.choice((0, rng.randrange(0, 10000))), rng.choice((sizes(rng), (1 << 32) - rng.randrange(0, 3))),
                               rng.choice((REC, REC16))]))
        c.append(("cache_arena", [rng.choice((sizes(rng), rng.randrange(1 << 25, 1 << 29))), rng.choice((0, rng.randrange(0, 288 << 30))), rng.choice((M64, M64, 0, 1, 64, 1 << 16))]))
    return c


@pytest.fixture(scope="module")
def cases():
    """every case once, with the answer by the rule: shared by the two tests and left alone"""
    return [(fn, args, RULES[fn](*args)) for fn, args in named_cases() + random_cases()]


def test_the_header_decides_as_the_drivers_did(cases):
    L = C.CDLL(build_harness.build_stage_b_plan())
    L.sbp_eval.restype = C.c_long
    L.sbp_eval.argtypes = [C.c_char_p, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.c_uint64), C.c_size_t]
    out = (C.c_uint64 * 256)()
    counts = {}
    for fn, args, want in cases:
        arr = (C.c_uint64 * max(1, len(args)))(*args)
        n = L.sbp_eval(fn.encode(), arr, len(args), out, 256)
        assert n >= 0 and list(out[:n]) == want, (fn, args, list(out[:max(n, 0)]), want)
        counts[fn] = counts.get(fn, 0) + 1
    assert set(counts) == set(RULES) and all(v >= N_RANDOM for v in counts.values()), counts
    assert L.sbp_eval(b"no such function", out, 0, out, 256) == -1


def test_a_sanitizer_build_decides_the_same(cases, tmp_path):
    exe = os.path.join(NATIVE, "stage_b_plan_main")
    deps = [os.path.join(NATIVE, f) for f in ("stage_b_plan_main.cpp", "stage_b_plan_host.cpp")] + [os.path.join(ROOT, "stringsext_amd", "csrc", "sx_stage_b_plan.hpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in deps):
        tmp = f"{exe}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", tmp, deps[0]])
        os.replace(tmp, exe)
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        f.writelines("%s %s\n" % (fn, " ".join(map(str, args))) for fn, args, _ in cases)
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-3000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases)
    for line, (fn, args, want) in zip(lines, cases):
        assert [int(x) for x in line.split()] == want, (fn, args, line, want)
