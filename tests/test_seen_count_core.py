"""A seen set that counts (SX_SEEN_COUNTED), its counts read back per finding, and the selection by a field of a label word: the lane
functions (stringsext_amd/csrc/sx_seen_count_core.hpp) compiled as plain host C++ and driven the way sx_seen_count_dev.hip and the
entry points drive them (tests/native/seen_count_host.cpp: behind the result path's or the merge path's add pass one more pass, then
the host's check of the counted total), with a Python Counter carried across the calls as the model.  No expected value comes from the
code under test.  The harness builds its sets with the seven initialisers of tests/native/seen_set_host.hpp, so `counts` is NULL until
the test gives a set count words; those, and a list's count array, end where a page without access begins."""
import ctypes as C
import os
import random
import subprocess
from collections import Counter

import pytest

import stringsext_amd as sx
import test_seen_core
import test_seen_merge_core as tm
from test_distinct_core import fold
from test_select_core import records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "stringsext_amd", "csrc")
DEPS = tm.DEPS + [os.path.join(NATIVE, "seen_merge_host.cpp"), os.path.join(CSRC, "sx_seen_count_core.hpp")]
M32 = (1 << 32) - 1
RS, FS = sx.SX_SEEN_RESULTS_SHIFT, sx.SX_SEEN_FINDINGS_SHIFT
entry_bytes = tm.entry_bytes


def word(results, findings):
    return results << RS | findings << FS


def halves(w):
    return w >> RS & M32, w >> FS & M32


@pytest.fixture(scope="module")
def core():
    out, src = os.path.join(NATIVE, "libseen_count_host.so"), os.path.join(NATIVE, "seen_count_host.cpp")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in DEPS + [src]):
        tmp = f"{out}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O2", "-fPIC", "-shared", "-o", tmp, src])
        os.replace(tmp, out)
    L = C.CDLL(out)
    u64p, vp, vpp = C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_void_p)
    L.sxs_seen_new.restype, L.sxs_seen_new.argtypes = vp, [C.c_int32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64]
    L.sxs_seen_free.restype, L.sxs_seen_free.argtypes = None, [vp]
    L.sxs_seen_state.restype, L.sxs_seen_state.argtypes = None, [vp, u64p]
    L.sxs_seen_raw.restype, L.sxs_seen_raw.argtypes = None, [vp, u64p, C.c_char_p]
    L.sxs_seen_dump.restype, L.sxs_seen_dump.argtypes = C.c_uint64, [vp, u64p, u64p, u64p, C.c_uint64, C.c_char_p, C.c_uint64]
    L.sxm_list_new.restype, L.sxm_list_new.argtypes = vp, [u64p, C.c_uint64, C.c_char_p, C.c_uint64]
    L.sxm_list_free.restype, L.sxm_list_free.argtypes = None, [vp]
    L.sxs_guarded.restype, L.sxs_guarded.argtypes = C.c_void_p, [C.c_uint64, C.POINTER(C.c_void_p), u64p]
    L.sxs_unmap.restype, L.sxs_unmap.argtypes = None, [C.c_void_p, C.c_uint64]
    L.sxc_counts_new.restype, L.sxc_counts_new.argtypes = vp, [vp]
    L.sxc_counts_free.restype, L.sxc_counts_free.argtypes = None, [vp, vp]
    L.sxc_reset.restype, L.sxc_reset.argtypes = None, [vp, vp]
    L.sxc_counts_raw.restype, L.sxc_counts_raw.argtypes = None, [vp, u64p]
    L.sxc_sum.restype, L.sxc_sum.argtypes = C.c_uint64, [C.c_uint64, C.c_uint64]
    seg_args = [C.c_uint32, vpp, vpp, u64p, C.POINTER(C.c_int32)]
    L.sxc_seen_call.restype, L.sxc_seen_call.argtypes = C.c_int, [vp] + seg_args + [C.c_int32, C.c_uint32, C.c_uint32, vpp, u64p]
    L.sxs_seen_call = L.sxc_seen_call                      # (test_seen_core.HostSet.call binds this name: the call with its count pass)
    L.sxc_lookup.restype, L.sxc_lookup.argtypes = C.c_int, [vp] + seg_args + [C.c_uint32, vpp]
    L.sxc_merge_list.restype, L.sxc_merge_list.argtypes = C.c_int, [vp, vp, u64p, C.c_uint32, C.c_uint32, u64p, u64p]
    L.sxc_merge_set.restype, L.sxc_merge_set.argtypes = C.c_int, [vp, vp, C.c_uint32, C.c_uint32, u64p, u64p]
    L.sxc_range_pick.restype = C.c_int
    L.sxc_range_pick.argtypes = [vp, C.c_uint64, C.c_int32, u64p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_char_p, C.POINTER(C.c_uint32)]
    return L


class HostSet(tm.HostSet):
    """one set of the harness, which counts if it is told to"""

    def __init__(self, L, capacity_strings, capacity_bytes, table_log2=-1, tag_bits=24, nocase=False, counted=True):
        super().__init__(L, capacity_strings, capacity_bytes, table_log2, tag_bits, nocase)
        self.k = L.sxc_counts_new(self.h) if counted else None
        assert self.k or not counted

    def free(self):
        if self.k:
            self.L.sxc_counts_free(self.h, self.k)
        super().free()

    def reset(self):
        self.L.sxc_reset(self.h, self.k)

    def counts_raw(self):
        out = (C.c_uint64 * (1 << self.state()["table_log2"]))()
        self.L.sxc_counts_raw(self.k, out)
        return list(out)

    def counts(self):
        """{the stored string: (results, findings)}; the word of every empty slot is 0"""
        raw, dump = self.counts_raw(), self.dump()
        occupied = {slot for slot, _, _ in dump}
        assert all(w == 0 for s, w in enumerate(raw) if s not in occupied)
        return {s: halves(raw[slot]) for slot, _, s in dump}

    def merge(self, src, add=True, groups=2, counts=None):
        """as tm.HostSet.merge, with the count pass behind it; counts: a list source's count words"""
        L, info = self.L, (C.c_uint64 * 4)()
        if isinstance(src, tm.HostSet):
            held = (C.c_uint64 * (((1 << src.state()["table_log2"]) + 63) // 64))()
            return L.sxc_merge_set(self.h, src.h, groups, int(not add), held, info), dict(zip(tm.INFO, info))
        words, arena = src
        n = len(words)
        held = (C.c_uint64 * max(1, (n + 63) // 64))()
        lst = L.sxm_list_new((C.c_uint64 * max(1, n))(*words), n, arena, len(arena))
        assert lst
        try:
            arr = None if counts is None else (C.c_uint64 * max(1, n))(*counts)
            return L.sxc_merge_list(self.h, lst, arr, groups, int(not add), held, info), dict(zip(tm.INFO, info))
        finally:
            L.sxm_list_free(lst)

    def lookup(self, segments, groups=2, packed=True):
        """the count word of every finding's string, in print order (sx_result_seen_counts_device)"""
        L, n_segs = self.L, len(segments)
        regions, keep = [], []
        recs, arenas, labels = (C.c_void_p * n_segs)(), (C.c_void_p * n_segs)(), (C.c_void_p * n_segs)()
        ns, pk = (C.c_uint64 * n_segs)(), (C.c_int32 * n_segs)()
        try:
            for s, strings in enumerate(segments):
                arena, offs, at = b"".join(strings), [], 0
                for x in strings:
                    offs.append(at); at += len(x)
                region, region_bytes = C.c_void_p(), C.c_uint64()
                base = L.sxs_guarded(max(1, len(arena)), C.byref(region), C.byref(region_bytes))
                assert base
                regions.append((region, region_bytes))
                C.memmove(base, arena, len(arena))
                arr = records(strings, offs, packed)
                out = (C.c_uint64 * max(1, len(strings)))(*([0xEEEEEEEEEEEEEEEE] * max(1, len(strings))))
                keep += [arr, out]
                recs[s], arenas[s], labels[s], ns[s], pk[s] = C.addressof(arr), base, C.addressof(out), len(strings), int(packed)
            rc = L.sxc_lookup(self.h, n_segs, recs, arenas, ns, pk, groups, labels)
            return rc, [w for s, strings in enumerate(segments) for w in list(keep[2 * s + 1])[:len(strings)]]
        finally:
            for region, region_bytes in regions:
                L.sxs_unmap(region, region_bytes)


class Model:
    """{key: [results, findings]} carried across the calls; a key is a string under the set's fold"""

    def __init__(self, nocase=False):
        self.key = fold if nocase else (lambda s: s)
        self.c = {}

    def result(self, flat):
        """one result: results += 1 per class, findings += its size"""
        for k, n in Counter(self.key(s) for s in flat).items():
            self.add(k, 1, n)

    def add(self, k, results, findings):
        r, f = self.c.get(k, (0, 0))
        self.c[k] = (min(M32, r + results), min(M32, f + findings))

    def words(self, flat):
        return [word(*self.c[self.key(s)]) if self.key(s) in self.c else 0 for s in flat]

    def room(self):
        return max(1, len(self.c)), sum(entry_bytes(len(k)) for k in self.c)


def stream(rng):
    """three results with overlapping strings in both cases, a class of size 3 next to singletons in each"""
    pool = [b"Alpha", b"alpha", b"ALPHA", b"beta", b"Beta", b"", b"gamma gamma", b"k\xc0z", b"K\xc0Z", b"k\xe0z"] + [b"w%d" % k + b"x" * (k % 9) for k in range(60)]
    out = []
    for k in range(3):
        flat = rng.sample(pool, 30) + [b"thrice %d" % k] * 3 + [b"in every result"] + [b"Twice", b"twice"] + [b"solo %d" % k]
        rng.shuffle(flat)
        out.append(flat)
    return out


def room_for(results, nocase):
    m = Model(nocase)
    for flat in results:
        m.result(flat)
    return m.room()


@pytest.mark.parametrize("nocase", [False, True])
@pytest.mark.parametrize("tag_bits", [0, 24])
def test_three_results_in_a_row_against_a_counter(core, tag_bits, nocase):
    rng = random.Random(60 + tag_bits)
    results = stream(rng)
    cap_s, cap_b = room_for(results, nocase)
    hs, m = HostSet(core, cap_s, cap_b, tm.legal_log2(cap_s), tag_bits, nocase), Model(nocase)
    try:
        for k, flat in enumerate(results):
            before = hs.counts_raw()
            rc, _, _ = hs.call([flat], add=False, rng=rng)                                 # lookup-only: no count word moves
            assert rc == 0 and hs.counts_raw() == before
            segs = test_seen_core.cut(flat, 1 + k)
            rc, words, info = hs.call(segs, groups=1 + k, rng=rng)
            assert rc == 0, rc
            m.result(flat)
            assert hs.counts() == m.c, k
            assert info["distinct"] == len({m.key(s) for s in flat})
            rc, got = hs.lookup(segs, groups=2 - k % 2)
            assert rc == 0 and got == m.words(flat)
            stranger = [b"not in the set", flat[0], b"Not In The Set"]
            rc, got = hs.lookup([stranger])
            assert rc == 0 and got == [0, m.words([flat[0]])[0], 0]
        assert m.c[m.key(b"in every result")] == (3, 3) and m.c[m.key(b"thrice 1")] == (1, 3) and m.c[m.key(b"solo 2")] == (1, 1)
        assert m.c[m.key(b"twice")] == ((3, 6) if nocase else (3, 3))
        rc, _, info = hs.call([results[2]], rng=rng)                                       # nothing new, everything seen: the count pass still runs
        assert rc == 0 and info["added_strings"] == 0
        m.result(results[2])
        assert hs.counts() == m.c
        hs.reset()
        assert hs.counts_raw() == [0] * (1 << hs.state()["table_log2"]) and hs.dump() == []
        rc, _, _ = hs.call([results[0]], rng=rng)
        m = Model(nocase)
        m.result(results[0])
        assert rc == 0 and hs.counts() == m.c
    finally:
        hs.free()


@pytest.mark.parametrize("short", [(1, 0), (0, 8)])
def test_a_refused_call_leaves_every_count_word(core, short):
    rng = random.Random(61)
    results = stream(rng)
    cap_s, cap_b = room_for(results, False)
    hs, m = HostSet(core, cap_s - short[0], cap_b - short[1], tm.legal_log2(cap_s)), Model()
    try:
        for flat in results[:2]:
            assert hs.call([flat], rng=rng)[0] == 0
            m.result(flat)
        before = hs.raw(), hs.counts_raw()
        assert hs.call([results[2]], rng=rng)[0] == 1                                      # what is new does not fit
        assert (hs.raw(), hs.counts_raw()) == before and hs.counts() == m.c
        words, arena = tm.source(sorted({b"new to the set %d" % k for k in range(40)} | {results[0][0]}))
        rc, _ = hs.merge((words, arena))
        assert rc == 1 and (hs.raw(), hs.counts_raw()) == before
    finally:
        hs.free()


@pytest.mark.parametrize("nocase", [False, True])
@pytest.mark.parametrize("tag_bits", [0, 24])
def test_merges_counted_and_plain_and_growth_to_another_table(core, tag_bits, nocase):
    rng = random.Random(62 + tag_bits)
    results = stream(rng)
    cap_s, cap_b = room_for(results, nocase)
    a, b = HostSet(core, cap_s, cap_b, tag_bits=tag_bits, nocase=nocase), HostSet(core, cap_s, cap_b, tag_bits=tag_bits, nocase=nocase)
    plain = HostSet(core, cap_s, cap_b, tag_bits=tag_bits, nocase=nocase, counted=False)
    grown = HostSet(core, 4 * cap_s, 2 * cap_b, tag_bits=24 - tag_bits, nocase=nocase)
    ma, mb, mp = Model(nocase), Model(nocase), Model(nocase)
    try:
        for hs, m, flats in ((a, ma, results[:2]), (b, mb, results[1:]), (plain, mp, results[2:])):
            for flat in flats:
                assert hs.call([flat], rng=rng)[0] == 0
                m.result(flat)
        assert a.counts() == ma.c and b.counts() == mb.c
        before = a.counts_raw()
        assert a.merge(b, add=False)[0] == 0 and a.counts_raw() == before                  # lookup-only
        rc, info = a.merge(b, groups=3)                                                    # counted + counted: the counts add
        assert rc == 0 and info["source_strings"] == len(mb.c)
        for k, (r, f) in mb.c.items():
            ma.add(k, r, f)
        assert a.counts() == ma.c
        rc, _ = a.merge(plain)                                                             # plain -> counted: (1, 1) per string of the source
        assert rc == 0
        for k in mp.c:
            ma.add(k, 1, 1)
        assert a.counts() == ma.c
        before = plain.raw()
        rc, info = plain.merge(a)                                                          # counted -> plain: a plain merge, nothing else
        assert rc == 0 and info["source_strings"] == len(ma.c) and sorted(s for _, _, s in plain.dump()) == sorted(ma.c)
        rc, _ = grown.merge(a, groups=1)                                                   # growth: into a fresh counted set of another table
        assert rc == 0 and grown.state()["table_log2"] > a.state()["table_log2"]
        assert grown.counts() == ma.c
    finally:
        for hs in (a, b, plain, grown):
            hs.free()


def test_a_list_source_with_multiplicities_and_saturation_of_each_half(core):
    hs, m = HostSet(core, 64, 4096, tag_bits=1), Model()
    try:
        strings = sorted([b"once", b"five times", b"", b"nearly full results", b"nearly full findings", b"both nearly full"])
        words, arena = tm.source(strings, random.Random(63), empties=1)
        by_offset, o = {}, 0
        while o < len(arena):
            n = int.from_bytes(arena[o:o + 4], "little")
            by_offset[o // 8] = arena[o + 8:o + 8 + n]
            o += entry_bytes(n)
        want = {b"once": (1, 1), b"five times": (1, 5), b"": (1, 2), b"nearly full results": (M32 - 1, M32 - 1), b"nearly full findings": (7, M32 - 1),
                b"both nearly full": (M32 - 1, M32 - 1)}
        counts = [0xDEAD if w == tm.EMPTY else word(*want[by_offset[w & (1 << tm.OFFSET_BITS) - 1]]) for w in words]      # (an empty word's count is never read)
        rc, info = hs.merge((words, arena), counts=counts)
        assert rc == 0 and info["added_strings"] == len(strings)
        for k, (r, f) in want.items():
            m.add(k, r, f)
        assert hs.counts() == m.c
        # add twice: a result with one finding of each, then a list that says (1, 3) of each
        for step in range(2):
            if step == 0:
                assert hs.call([strings])[0] == 0
                m.result(strings)
            else:
                assert hs.merge((words, arena), counts=[word(1, 3)] * len(words))[0] == 0
                for k in strings:
                    m.add(k, 1, 3)
            assert hs.counts() == m.c, step
        got = hs.counts()
        assert got[b"nearly full results"] == (M32, M32) and got[b"both nearly full"] == (M32, M32)
        assert got[b"nearly full findings"] == (9, M32)                                    # the high half is full, the low half goes on counting
        assert got[b"once"] == (3, 5) and got[b"five times"] == (3, 9)
    finally:
        hs.free()
    for a, b in ((word(M32 - 1, 5), word(1, 1)), (word(M32, 0), word(1, M32)), (word(3, M32 - 2), word(M32, 5)), (0, 0), (word(M32, M32), word(M32, M32))):
        ra, fa = halves(a); rb, fb = halves(b)
        assert core.sxc_sum(a, b) == word(min(M32, ra + rb), min(M32, fa + fb)), (hex(a), hex(b))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 8 * 64 + 1])
def test_counts_around_a_wavefront_and_a_grid_that_strides(core, n):
    """n distinct strings, every other one already held, as a result and as a list; 8 x 64 + 1: one more than a trip of one workgroup"""
    strings = [b"s%d" % k + b"y" * (k % 13) for k in range(n)]
    for groups in (1, 2):
        hs, m = HostSet(core, 2 * n + 2, 64 * n + 64, tag_bits=1), Model()
        try:
            assert hs.call([strings[::2]], groups=groups)[0] == 0
            m.result(strings[::2])
            flat = strings + strings[:n // 3]                                              # classes of 2 in front, seen and new alternate
            assert hs.call([flat], groups=groups)[0] == 0
            m.result(flat)
            assert hs.counts() == m.c
            words, arena = tm.source(strings, random.Random(n))
            assert hs.merge((words, arena), groups=groups)[0] == 0
            for k in strings:
                m.add(k, 1, 1)
            assert hs.counts() == m.c
            rc, got = hs.lookup([flat], groups=groups)
            assert rc == 0 and got == m.words(flat)
        finally:
            hs.free()


def test_the_selection_by_a_field_of_a_label_word(core):
    rng = random.Random(64)
    edge = [0, 1, 2, 4, 5, 6, M32 - 1, M32, M32 + 1, 1 << 32, 5 << 32, (5 << 32) - 1, (5 << 32) + 1, 1 << 63, (1 << 63) - 1, (1 << 64) - 1, (1 << 64) - 2]
    for n in (1, 63, 64, 65, 200):
        labels = [rng.choice(edge) if rng.random() < 0.7 else rng.getrandbits(64) for _ in range(n)]
        strings = [b"r" * (1 + k % 17) for k in range(n)]
        for packed in (True, False):
            arr = records(strings, [0] * n, packed)
            for shift, bits, lo, hi in ((0, 1, 1, 1), (0, 1, 0, 0), (63, 1, 1, 1), (5, 1, 0, 1), (0, 32, 2, M32), (32, 32, 5, M32), (32, 32, 5, 5), (32, 32, 0, 0),
                                        (16, 32, 1 << 16, 1 << 17), (0, 64, 0, (1 << 64) - 1), (0, 64, 1 << 63, (1 << 64) - 1), (0, 64, (1 << 64) - 1, (1 << 64) - 1),
                                        (0, 64, 6, 4), (32, 32, M32, 0), (0, 32, M32, M32), (1, 63, 0, 2), (61, 3, 4, 7)):
                sel, ln = C.create_string_buffer(n), (C.c_uint32 * n)()
                rc = core.sxc_range_pick(C.addressof(arr), n, int(packed), (C.c_uint64 * n)(*labels), shift, bits, lo, hi, sel, ln)
                assert rc == 0
                want = [lo <= (w >> shift & (1 << bits) - 1) <= hi for w in labels]
                assert [b != 0 for b in sel.raw] == want, (shift, bits, lo, hi)
                assert list(ln) == [len(s) if w else 0 for s, w in zip(strings, want)]


# ---- the same lane functions under the address and undefined-behaviour sanitizers, as a program of their own

def test_a_sanitizer_build_adds_merges_and_grows_the_same():
    exe, src = os.path.join(NATIVE, "seen_count_main"), os.path.join(NATIVE, "seen_count_main.cpp")
    deps = DEPS + [src, os.path.join(NATIVE, "seen_count_host.cpp")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in deps):
        tmp = f"{exe}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", tmp, src])
        os.replace(tmp, exe)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-500:], out.stderr[-2000:])
