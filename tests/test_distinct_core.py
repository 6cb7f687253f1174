"""The duplicate strings of a device-resident result (sx_result_distinct_device): the lane functions (stringsext_amd/csrc/
sx_distinct_core.hpp) compiled as plain host C++ and driven the way sx_distinct_dev.hip and the entry point drive them
(tests/native/distinct_core_host.cpp: per round the table emptied, claim over every segment's wavefronts, then resolve with one add
per wavefront, until the counter is 0, then finalize), against a Python dict over the strings.  No expected value comes from the
code under test.  Every segment's arena ends where a page without access begins: the core may read nothing behind the last string.
Every input runs with a table of 1, 2 and 16 slots and with the default: the words are the same whatever the table makes of the
rounds, and one slot means a round per distinct string."""
import collections
import ctypes as C
import os
import random
import subprocess

import pytest

import stringsext_amd as sx
from test_select_core import lay_out, records, text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "stringsext_amd", "csrc")
DEPS = [os.path.join(ROOT, "include", "stringsext_amd.h"), os.path.join(NATIVE, "seen_set_host.hpp"), os.path.join(NATIVE, "guarded_host.hpp")] + [os.path.join(CSRC, f) for f in (
    "sx_seen_core.hpp", "sx_distinct_core.hpp", "sx_select_core.hpp", "sx_seltally_core.hpp")]
FIRST, REPEATED, SHIFT = sx.SX_DISTINCT_FIRST, sx.SX_DISTINCT_REPEATED, sx.SX_DISTINCT_COUNT_SHIFT
TABLES = (0, 1, 4, -1)          # table_log2; -1: the default, the power of two >= 2 x findings


def built(out, src, flags):
    """(as tests/test_label_core.py builds its harness: g++ on one file, rebuilt when a source is newer)"""
    out, src = os.path.join(NATIVE, out), os.path.join(NATIVE, src)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in DEPS + [src]):
        tmp = f"{out}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + ["-o", tmp, src])
        os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def core():
    L = C.CDLL(built("libdistinct_core_host.so", "distinct_core_host.cpp", ["-O2", "-fPIC", "-shared"]))
    u64p, vpp = C.POINTER(C.c_uint64), C.POINTER(C.c_void_p)
    L.sxs_distinct_host.restype = C.c_int
    L.sxs_distinct_host.argtypes = [C.c_uint32, vpp, vpp, u64p, C.POINTER(C.c_int32), C.c_uint32, C.c_int32, C.c_uint32, vpp, u64p, u64p, C.c_uint32]
    L.sxs_distinct_slot.restype = C.c_uint64
    L.sxs_distinct_slot.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    L.sxs_guarded.restype, L.sxs_guarded.argtypes = C.c_void_p, [C.c_uint64, C.POINTER(C.c_void_p), u64p]
    L.sxs_unmap.restype, L.sxs_unmap.argtypes = None, [C.c_void_p, C.c_uint64]
    return L


def fold(s):
    """'A'..'Z' as 'a'..'z', no other byte"""
    return bytes(b | 0x20 if 0x41 <= b <= 0x5A else b for b in s)


def want_words(strings, nocase=False):
    """(the words in print order, distinct, repeated) from a dict over the strings"""
    keys = [fold(s) if nocase else s for s in strings]
    size = collections.Counter(keys)
    seen, words = set(), []
    for k in keys:
        words.append((FIRST if k not in seen else 0) | (REPEATED if size[k] > 1 else 0) | min(size[k], 0xFFFFFFFF) << SHIFT)
        seen.add(k)
    return words, len(size), sum(1 for c in size.values() if c > 1)


def decided(strings, nocase=False):
    """the input cannot hide an empty comparison: duplicates and singletons, a class of three or more"""
    size = collections.Counter(fold(s) if nocase else s for s in strings)
    assert 0 < len(size) < len(strings) and max(size.values()) >= 3 and min(size.values()) == 1, (len(size), len(strings))


def run(L, segments, nocase=False, table_log2=-1, packed=True, layout="packed", groups=2, rng=None):
    """the harness over `segments` (lists of strings); returns (the words in print order, info as a dict, the counter after each round)"""
    rng = rng or random.Random(len(segments))
    n_segs = len(segments)
    packed = [packed] * n_segs if isinstance(packed, bool) else list(packed)
    regions, keep = [], []
    recs, arenas, labels = (C.c_void_p * n_segs)(), (C.c_void_p * n_segs)(), (C.c_void_p * n_segs)()
    ns, pk = (C.c_uint64 * n_segs)(), (C.c_int32 * n_segs)()
    try:
        for s, strings in enumerate(segments):
            offs, arena = lay_out(strings, layout, rng)
            region, region_bytes = C.c_void_p(), C.c_uint64()
            base = L.sxs_guarded(max(1, len(arena)), C.byref(region), C.byref(region_bytes))
            assert base
            regions.append((region, region_bytes))
            C.memmove(base, arena, len(arena))
            arr = records(strings, offs, packed[s])
            out = (C.c_uint64 * max(1, len(strings)))(*([0xEEEEEEEEEEEEEEEE] * max(1, len(strings))))
            keep += [arr, out]
            recs[s], arenas[s], labels[s], ns[s], pk[s] = C.addressof(arr), base, C.addressof(out), len(strings), int(packed[s])
        info, left = (C.c_uint64 * 5)(), (C.c_uint64 * 4096)()
        rc = L.sxs_distinct_host(n_segs, recs, arenas, ns, pk, int(nocase), table_log2, groups, labels, info, left, 4096)
        assert rc == 0, rc
        words = [w for s, strings in enumerate(segments) for w in list(keep[2 * s + 1])[:len(strings)]]
        info = dict(findings=info[0], distinct=info[1], repeated=info[2], rounds=info[3], table_log2=info[4])
        return words, info, list(left)[:min(info["rounds"], 4096)]
    finally:
        for region, region_bytes in regions:
            L.sxs_unmap(region, region_bytes)


def check(L, segments, nocase=False, every=True):
    """`segments` at every table size, packed and unpacked records, both layouts, against the dict"""
    flat = [s for seg in segments for s in seg]
    decided(flat, nocase)
    want, distinct, repeated = want_words(flat, nocase)
    for packed, layout in (((True, "packed"), (False, "scattered"), (False, "packed")) if every else ((True, "packed"),)):
        for log2 in TABLES:
            got, info, left = run(L, segments, nocase, log2, packed, layout, groups=1 + len(flat) % 3)
            assert got == want, (log2, packed, layout, [(i, flat[i], hex(got[i]), hex(want[i])) for i in range(len(flat)) if got[i] != want[i]][:5])
            assert (info["findings"], info["distinct"], info["repeated"]) == (len(flat), distinct, repeated), info
            want_log2 = log2 if log2 >= 0 else next(p for p in range(1, 64) if 1 << p >= 2 * len(flat))
            assert info["table_log2"] == want_log2
            assert 1 <= info["rounds"] <= distinct and (log2 != 0 or info["rounds"] == distinct), (log2, info)
            assert all(a > b for a, b in zip([len(flat)] + left, left)) and left[-1] == 0, left       # every round makes progress
            again = run(L, segments, nocase, log2, packed, layout, groups=3)
            assert (again[0], again[1], again[2]) == (got, info, left)                               # the rounds do not depend on the grid or the run
    return want


def words_with_repeats(rng, n, alphabet=b"abcdefghijklmnopqrstuvwxyz0123456789 /_.-"):
    """n random words, of which about a third are planted again, some of them many times"""
    pool = [text(rng, rng.randrange(1, 40), alphabet) for _ in range(max(2, n // 2))]
    heavy = pool[:3]
    out = [rng.choice(heavy) if rng.random() < 0.15 else rng.choice(pool) if rng.random() < 0.4 else text(rng, rng.randrange(1, 40), alphabet) + b"#%d" % i
           for i in range(n)]
    out[rng.randrange(n)] = b"only once, surely: " + bytes([rng.randrange(256) for _ in range(8)])
    return out


def test_random_words_with_planted_repeats(core):
    rng = random.Random(20)
    check(core, [words_with_repeats(rng, 400)])
    check(core, [words_with_repeats(rng, 300, alphabet=bytes(range(256)))])


def test_empty_strings_are_one_class(core):
    rng = random.Random(21)
    strings = words_with_repeats(rng, 200)
    for k in (0, 5, 70, 199):
        strings[k] = b""
    want = check(core, [strings])
    assert want[0] == FIRST | REPEATED | 4 << SHIFT and want[199] == REPEATED | 4 << SHIFT
    check(core, [[b""] * 70 + [b"a", b"b", b"a", b"a"]])


def test_strings_that_differ_in_their_last_byte_only_and_prefixes_of_one_another(core):
    rng = random.Random(22)
    stem = text(rng, 90, b"abcdefgh")
    strings = [stem + bytes([65 + k % 7]) for k in range(150)]                 # seven classes that part at the last byte
    strings += [stem[:k] for k in range(0, 91)] + [stem[:k] for k in range(0, 91, 3)] + [stem[:30]] * 2      # every prefix, the empty one too
    strings += [stem + b"\x00", stem + b"\x00\x00", stem + b"\x00"]
    rng.shuffle(strings)
    strings.append(b"a singleton")
    check(core, [strings])


def test_letter_case_with_and_without_the_fold(core):
    rng = random.Random(23)
    base = [text(rng, rng.randrange(3, 20), b"abcdXYZ9_") for _ in range(120)]
    strings = []
    for s in base:
        strings += [s, s.upper() if rng.random() < 0.5 else s.lower(), s.swapcase()][:rng.randrange(1, 4)]
    strings += [b"Ab", b"aB", b"AB", b"ab", b"ab", b"ab", b"lonely \xc3\x84"]
    plain = check(core, [strings])
    folded = check(core, [strings], nocase=True)
    assert sum(w & FIRST for w in folded) < sum(w & FIRST for w in plain)      # the fold joins classes
    at = strings.index(b"Ab")
    assert folded[at] >> SHIFT >= 6 and plain[at] >> SHIFT >= 1 and plain[strings.index(b"ab")] >> SHIFT >= 3


def test_the_fold_touches_no_byte_from_0x80_on_nor_the_neighbours_of_the_letters(core):
    strings = []
    for a, b in ((0xC0, 0xE0), (0xC4, 0xE4), (0x81, 0xA1), (0x9A, 0xBA), (0x40, 0x60), (0x5B, 0x7B), (0x5E, 0x7E), (0x00, 0x20)):   # 0x20 apart, no letters
        strings += [b"k" + bytes([a]) + b"z", b"K" + bytes([b]) + b"Z", b"k" + bytes([a]) + b"Z"]
    strings += [b"\xc3\x84rger", b"\xc3\xa4rger", b"\xc3\x84RGER", b"\xc3\x84rger", b"solo"]
    want = check(core, [strings], nocase=True)
    # k<a>z and k<a>Z are one class, K<b>Z is another: six strings give two classes of sizes 2 and 1 per pair
    assert [w >> SHIFT for w in want[:3]] == [2, 1, 2] and want[1] & FIRST
    assert [w >> SHIFT for w in want[-5:-1]] == [3, 1, 3, 3]
    check(core, [strings + [b"solo", b"solo"]])


@pytest.mark.parametrize("n_segs", [2, 3])
def test_classes_that_span_segments_of_packed_and_unpacked_records(core, n_segs):
    rng = random.Random(24 + n_segs)
    flat = words_with_repeats(rng, 500)
    cuts = sorted(rng.sample(range(100, 400), n_segs - 1))
    segments = [flat[a:b] for a, b in zip([0] + cuts, cuts + [500])]
    shared = b"in every segment"
    for seg in segments:
        seg[rng.randrange(len(seg))] = shared
    flat = [s for seg in segments for s in seg]
    want, _, _ = want_words(flat)
    at = [i for i, s in enumerate(flat) if s == shared]
    assert [want[i] for i in at] == [FIRST | REPEATED | n_segs << SHIFT] + [REPEATED | n_segs << SHIFT] * (n_segs - 1)
    check(core, segments)
    for packed in ([True, False, True][:n_segs], [False, True, False][:n_segs]):       # segments of both record types in one result
        got, info, _ = run(core, segments, packed=packed, layout="scattered", rng=rng)
        assert got == want and info["distinct"] == len(set(flat))


@pytest.mark.parametrize("n", [63, 64, 65])
def test_record_counts_around_a_wavefront(core, n):
    rng = random.Random(25 + n)
    strings = words_with_repeats(rng, n)
    strings[-1] = strings[0] = strings[n // 2] = b"first, middle and last"
    strings[1] = b"alone"
    want = check(core, [strings])
    assert want[-1] == REPEATED | 3 << SHIFT


def test_one_record_alone_and_as_a_segment_of_its_own(core):
    """n = 1 has one class of one: it cannot meet check()'s "0 < distinct < n", so its word is spelt out here, and the one-record
    segment is checked in full next to segments of 63, 64 and 65 records"""
    for log2 in TABLES:
        for packed in (True, False):
            got, info, left = run(core, [[b"the only one"]], table_log2=log2, packed=packed)
            assert got == [FIRST | 1 << SHIFT] and left == [0]
            assert info == dict(findings=1, distinct=1, repeated=0, rounds=1, table_log2=max(log2, 1) if log2 else 0)
    rng = random.Random(26)
    flat = words_with_repeats(rng, 193)
    flat[0] = flat[63] = flat[192] = b"the only one"
    check(core, [flat[:1], flat[1:64], flat[64:128], flat[128:]])


def test_every_round_spreads_the_strings_anew(core):
    """the seed matters: strings that share a slot in round 0 mostly part in round 1 (nothing rests on it but the number of rounds)"""
    rng = random.Random(27)
    strings = sorted({text(rng, rng.randrange(1, 30), b"abcdefghij") for _ in range(2000)})
    slots = [[core.sxs_distinct_slot(s, len(s), 0, r, 8) for s in strings] for r in (0, 1)]
    assert all(0 <= x < 256 for r in slots for x in r) and len(set(slots[0])) > 200
    pairs = [(i, j) for i in range(0, len(strings), 7) for j in range(i + 1, min(i + 40, len(strings))) if slots[0][i] == slots[0][j]]
    assert len(pairs) > 20 and sum(1 for i, j in pairs if slots[1][i] == slots[1][j]) < len(pairs) // 4
    assert core.sxs_distinct_slot(b"MiXed", 5, 1, 3, 20) == core.sxs_distinct_slot(b"mixed", 5, 1, 3, 20)
    assert core.sxs_distinct_slot(b"MiXed", 5, 0, 3, 20) != core.sxs_distinct_slot(b"mixed", 5, 0, 3, 20)
    assert core.sxs_distinct_slot(b"anything", 8, 0, 5, 0) == 0
