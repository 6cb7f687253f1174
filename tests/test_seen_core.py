"""The seen set of device-resident results (sx_seen_set, sx_result_seen_device): the lane functions (stringsext_amd/csrc/
sx_seen_core.hpp, and the distinct core in front of them) compiled as plain host C++ and driven the way sx_seen_dev.hip and the entry
point drive them (tests/native/seen_core_host.cpp: the distinct pass under the set's fold, mark over every segment, the host's look at
the totals, add over every segment) over a SEQUENCE of results against one set, with a Python set carried across the calls as the
model and want_words of tests/test_distinct_core.py for bits 0, 1 and 32..63.  No expected value comes from the code under test.
Every arena — the sources' and the set's — ends where a page without access begins.  The harness takes table_log2 and tag_bits as
they are: tables of 2 and 4 slots make every probe a chain, tag_bits 0 and 1 make the tags collide."""
import ctypes as C
import os
import random
import subprocess

import pytest

import stringsext_amd as sx
from test_distinct_core import fold, want_words, words_with_repeats
from test_select_core import lay_out, records, text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "stringsext_amd", "csrc")
DEPS = [os.path.join(ROOT, "include", "stringsext_amd.h"), os.path.join(NATIVE, "distinct_core_host.cpp"), os.path.join(NATIVE, "seen_set_host.hpp"), os.path.join(NATIVE, "guarded_host.hpp")] + [os.path.join(CSRC, f) for f in (
    "sx_seen_core.hpp", "sx_distinct_core.hpp", "sx_select_core.hpp", "sx_seltally_core.hpp")]
FIRST, REPEATED, SEEN, SHIFT = sx.SX_DISTINCT_FIRST, sx.SX_DISTINCT_REPEATED, sx.SX_DISTINCT_SEEN, sx.SX_DISTINCT_COUNT_SHIFT
INFO = ("findings", "distinct", "repeated", "seen_findings", "seen_distinct", "added_strings", "added_bytes", "rounds", "table_log2")
TAGS = (0, 1, 24)
LAYOUTS = ((True, "packed"), (False, "scattered"), (False, "packed"))      # (packed records, the strings' layout)


def entry_bytes(n):
    """SX_SEEN_ENTRY_BYTES"""
    return 8 + (n + 7) // 8 * 8


def legal_log2(capacity_strings):
    """the power of two >= 2 x capacity_strings, at least 2 slots"""
    return next(p for p in range(1, 64) if 1 << p >= 2 * capacity_strings)


@pytest.fixture(scope="module")
def core():
    out, src = os.path.join(NATIVE, "libseen_core_host.so"), os.path.join(NATIVE, "seen_core_host.cpp")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in DEPS + [src]):
        tmp = f"{out}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O2", "-fPIC", "-shared", "-o", tmp, src])
        os.replace(tmp, out)
    L = C.CDLL(out)
    u64p, vpp, vp = C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.c_void_p
    L.sxs_seen_new.restype, L.sxs_seen_new.argtypes = vp, [C.c_int32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64]
    L.sxs_seen_free.restype, L.sxs_seen_free.argtypes = None, [vp]
    L.sxs_seen_reset.restype, L.sxs_seen_reset.argtypes = None, [vp]
    L.sxs_seen_state.restype, L.sxs_seen_state.argtypes = None, [vp, u64p]
    L.sxs_seen_dump.restype, L.sxs_seen_dump.argtypes = C.c_uint64, [vp, u64p, u64p, u64p, C.c_uint64, C.c_char_p, C.c_uint64]
    L.sxs_seen_home.restype, L.sxs_seen_home.argtypes = C.c_uint64, [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32]
    L.sxs_seen_tag.restype, L.sxs_seen_tag.argtypes = C.c_uint64, [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32]
    L.sxs_seen_call.restype = C.c_int
    L.sxs_seen_call.argtypes = [vp, C.c_uint32, vpp, vpp, u64p, C.POINTER(C.c_int32), C.c_int32, C.c_uint32, C.c_uint32, vpp, u64p]
    L.sxs_guarded.restype, L.sxs_guarded.argtypes = C.c_void_p, [C.c_uint64, C.POINTER(C.c_void_p), u64p]
    L.sxs_unmap.restype, L.sxs_unmap.argtypes = None, [C.c_void_p, C.c_uint64]
    return L


class HostSet:
    """one set of the harness"""

    def __init__(self, L, capacity_strings, capacity_bytes, table_log2=-1, tag_bits=24, nocase=False):
        self.L, self.nocase = L, nocase
        self.h = L.sxs_seen_new(table_log2, tag_bits, int(nocase), capacity_strings, capacity_bytes)
        assert self.h

    def free(self):
        self.L.sxs_seen_free(self.h)

    def reset(self):
        self.L.sxs_seen_reset(self.h)

    def state(self):
        out = (C.c_uint64 * 6)()
        self.L.sxs_seen_state(self.h, out)
        return dict(zip(("strings", "bytes", "capacity_strings", "capacity_bytes", "table_log2", "tag_bits"), out))

    def dump(self):
        """[(slot, word, the stored string)] by a walk over the table"""
        st = self.state()
        cap = 1 << st["table_log2"]
        slot, word, ln = (C.c_uint64 * cap)(), (C.c_uint64 * cap)(), (C.c_uint64 * cap)()
        buf = C.create_string_buffer(st["bytes"] + 8)
        n = self.L.sxs_seen_dump(self.h, slot, word, ln, cap, buf, st["bytes"] + 8)
        assert n <= cap, "an entry that does not fit its arena, or whose second word is not 0"
        out, at = [], 0
        for k in range(n):
            out.append((slot[k], word[k], buf.raw[at:at + ln[k]]))
            at += (ln[k] + 7) // 8 * 8
        return out

    def call(self, segments, add=True, packed=True, layout="packed", groups=2, distinct_log2=-1, rng=None):
        """(the harness's code, the words in print order, info as a dict)"""
        L = self.L
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
            info = (C.c_uint64 * 9)()
            rc = L.sxs_seen_call(self.h, n_segs, recs, arenas, ns, pk, distinct_log2, groups, int(not add), labels, info)
            words = [w for s, strings in enumerate(segments) for w in list(keep[2 * s + 1])[:len(strings)]]
            return rc, words, dict(zip(INFO, info))
        finally:
            for region, region_bytes in regions:
                L.sxs_unmap(region, region_bytes)


class Model:
    """a Python set carried across the calls"""

    def __init__(self, nocase=False):
        self.nocase, self.held = nocase, set()

    def call(self, flat, add=True):
        """(the words, the first seven fields of info); with add the set then holds the strings"""
        keys = [fold(s) if self.nocase else s for s in flat]
        words, distinct, repeated = want_words(flat, self.nocase)
        words = [w | (SEEN if k in self.held else 0) for w, k in zip(words, keys)]
        classes = list(dict.fromkeys(keys))
        new = [k for k in classes if k not in self.held]
        info = dict(findings=len(flat), distinct=distinct, repeated=repeated, seen_findings=sum(k in self.held for k in keys),
                    seen_distinct=len(classes) - len(new), added_strings=len(new) if add else 0, added_bytes=sum(entry_bytes(len(k)) for k in new) if add else 0)
        if add:
            self.held |= set(new)
        return words, info

    def bytes(self):
        return sum(entry_bytes(len(k)) for k in self.held)


def decided(all_words):
    """the sequence cannot hide an empty comparison: findings that are seen and first, seen and not first, new and repeated, and new
    singletons"""
    kinds = {(bool(w & SEEN), bool(w & FIRST), w >> SHIFT > 1) for w in all_words}
    assert {(True, True), (True, False)} <= {k[:2] for k in kinds} and (False, True, True) in kinds and (False, True, False) in kinds, kinds


def cut(strings, n_segs):
    """n_segs segments of nearly the same size"""
    n = len(strings)
    assert n >= n_segs
    return [strings[n * k // n_segs:n * (k + 1) // n_segs] for k in range(n_segs)]


def capacity_of(steps, nocase=False):
    """(strings, bytes) that exactly hold what the steps add"""
    m = Model(nocase)
    for strings, add in steps:
        m.call(strings, add)
    return len(m.held), m.bytes()


def run_sequence(L, steps, capacity=None, table_log2=-1, tag_bits=24, nocase=False, packed=True, layout="packed", n_segs=1, groups=2, decides=True):
    """steps = [(strings, add)] against one set (capacity None: exactly what they add) and the model, everything compared after every
    step; returns ([the words of every step], [the infos], the set's dump at the end)"""
    exact = capacity is None
    cap_s, cap_b = capacity_of(steps, nocase) if exact else capacity
    hs, m = HostSet(L, max(1, cap_s), cap_b, table_log2, tag_bits, nocase), Model(nocase)
    try:
        all_words, infos = [], []
        for k, (strings, add) in enumerate(steps):
            want, want_info = m.call(strings, add)
            rc, got, info = hs.call(cut(strings, min(n_segs, len(strings))), add, packed, layout, groups, rng=random.Random(k))
            assert rc == 0, (k, rc)
            assert got == want, (k, [(i, strings[i], hex(got[i]), hex(want[i])) for i in range(len(strings)) if got[i] != want[i]][:5])
            assert {f: info[f] for f in want_info} == want_info, (k, info, want_info)
            st, dump = hs.state(), hs.dump()
            assert (st["strings"], st["bytes"]) == (len(m.held), m.bytes()), (k, st)
            assert sorted(s for _, _, s in dump) == sorted(m.held), k                      # each once, folded, nothing else
            assert len({w & (1 << 40) - 1 for _, w, _ in dump}) == len(dump)              # every slot its own entry
            all_words += want
            infos.append(info)
        if decides:
            decided(all_words)
        if exact and any(add for _, add in steps) and cap_s:
            assert (st["strings"], st["bytes"]) == (st["capacity_strings"], st["capacity_bytes"])        # filled to 100 %
        return all_words, infos, dump
    finally:
        hs.free()


def three_results(rng, n=150):
    """three results with overlapping and fresh strings; classes span any cut"""
    a = words_with_repeats(rng, n)
    b = rng.sample(a, n // 3) + [a[0], a[0], a[1]] + words_with_repeats(rng, n)
    rng.shuffle(b)
    c = rng.sample(a, n // 5) + rng.sample(b, n // 4) + [b[0]] * 3 + words_with_repeats(rng, n // 2)
    rng.shuffle(c)
    return [(a, True), (b, True), (c, True)]


@pytest.mark.parametrize("tag_bits", TAGS)
@pytest.mark.parametrize("n_segs", [1, 2, 3])
def test_three_results_in_a_row_at_the_smallest_legal_and_the_default_table(core, tag_bits, n_segs):
    rng = random.Random(40 + n_segs)
    steps = three_results(rng)
    cap_s, cap_b = capacity_of(steps)
    for packed, layout in LAYOUTS:
        # exactly what the steps add: the smallest table the entry point may make, at load 1/2 or a little less, filled to 100 %
        one = run_sequence(core, steps, None, legal_log2(cap_s), tag_bits, packed=packed, layout=layout, n_segs=n_segs, groups=1 + n_segs % 2)
        # room to spare, the table by the entry point's rule
        two = run_sequence(core, steps, (4 * cap_s, 3 * cap_b), -1, tag_bits, packed=packed, layout=layout, n_segs=n_segs)
        assert one[0] == two[0] and [{k: v for k, v in i.items() if k != "table_log2"} for i in one[1]] == [{k: v for k, v in i.items() if k != "table_log2"} for i in two[1]]
    flat = steps[1][0]
    if n_segs > 1:      # a class whose first and a later member lie in different segments
        seg_of = [k for k, seg in enumerate(cut(flat, n_segs)) for _ in seg]
        first = {}
        assert any(first.setdefault(s, k) != k for s, k in zip(flat, seg_of))


@pytest.mark.parametrize("tag_bits", TAGS)
def test_tables_of_two_and_of_four_slots(core, tag_bits):
    """(the harness takes the table as it is told: one slot stays empty, so every probe ends; every lookup walks a chain)"""
    a, b, c, d, e = b"alpha", b"beta", b"gamma gamma", b"", b"epsilon."
    two = [([a, a], True), ([a, b, b, a, c], False), ([a, a, a], True)]
    four = [([a, b, a], True), ([b, c, c, b, a], True), ([c, d, a, e, e], False)]
    for packed, layout in LAYOUTS:
        for n_segs in (1, 2, 3):
            _, _, dump = run_sequence(core, two, (1, 64), 1, tag_bits, packed=packed, layout=layout, n_segs=n_segs)
            assert [s for _, _, s in dump] == [a]
            _, _, dump = run_sequence(core, four, (3, 256), 2, tag_bits, packed=packed, layout=layout, n_segs=n_segs)
            assert sorted(s for _, _, s in dump) == sorted([a, b, c]) and len({slot for slot, _, _ in dump}) == 3


@pytest.mark.parametrize("tag_bits", TAGS)
def test_an_adder_that_finds_no_slot_is_an_error(core, tag_bits):
    """Three pairwise different new strings in ONE call into an empty set whose table was given 2 slots, with room for 3 strings: the mark
    pass meets only empty slots, so the call reaches the add pass, whose third claim walks both slots and finds none.  The call answers
    -3, as a merge does; it used to answer 0 over cursors that said 3 strings and a table that held 2."""
    hs = HostSet(core, 3, 256, 1, tag_bits)
    try:
        rc, words, info = hs.call([[b"alpha", b"beta", b"gamma gamma"]])
        st = hs.state()
        print("rc", rc, "cursor strings", st["strings"], "occupied slots", len(hs.dump()))
        assert rc == -3
        assert (info["seen_findings"], info["added_strings"]) == (0, 3)      # mark saw nothing and counted three new classes
    finally:
        hs.free()


def test_a_probe_that_wraps_around_the_end_of_the_table(core):
    log2 = 3
    last = [b"w%d" % k for k in range(400) if core.sxs_seen_home(b"w%d" % k, len(b"w%d" % k), 0, log2) == (1 << log2) - 1]
    assert len(last) >= 6
    steps = [(last[:3], True), ([last[0], last[3], last[3], last[0], last[4], last[2]], False), ([last[1], last[5]], True)]
    for tag_bits in TAGS:
        _, _, dump = run_sequence(core, steps, (4, 64), log2, tag_bits)
        assert sorted(slot for slot, _, _ in dump) == [0, 1, 2, 7]                    # the last slot, then the table's first three
        assert {s for slot, _, s in dump if slot == 2} == {last[5]}


def test_the_empty_string_is_seen_only_after_it_was_added(core):
    for tag_bits in TAGS:
        words, _, _ = run_sequence(core, [([b"x", b"", b"y", b"", b"y"], False), ([b"", b"x", b""], True), ([b"", b"x", b"z", b"z", b"", b"q"], True)], tag_bits=tag_bits)
        assert words[1] == FIRST | REPEATED | 2 << SHIFT                                  # looked up in the empty set
        assert words[5] == FIRST | REPEATED | 2 << SHIFT                                  # the set is still empty: the first step added nothing
        assert words[8] == FIRST | REPEATED | SEEN | 2 << SHIFT and words[12] == REPEATED | SEEN | 2 << SHIFT


def test_prefixes_of_one_another_last_bytes_and_the_padding_region(core):
    rng = random.Random(43)
    stem = text(rng, 40, b"abcdefgh")
    prefixes = [stem[:k] for k in range(0, 41)]
    ends = [stem + bytes([65 + k]) for k in range(7)]                                    # they part at the last byte
    pads = [b"1234567", b"12345678", b"123456789", b"1234567\x00", b"12345678\x00", b"1234567\x00\x00", b"1234567\x01"]     # len 7, 8, 9: what differs lies where a shorter one's padding is
    nul = [b"a\x00", b"a"]
    first = prefixes[::2] + ends[::2] + pads[:3] + nul[:1]
    second = prefixes + ends + pads + nul + [prefixes[2], ends[1], ends[1], b"a\x00\x00"]
    rng.shuffle(second)
    for tag_bits in TAGS:
        words, _, _ = run_sequence(core, [(first, True), (second, True), (second, False)], tag_bits=tag_bits, layout="scattered", packed=False)
        by = dict(zip(second, words[len(first):len(first) + len(second)]))
        assert by[b"a\x00"] & SEEN and not by[b"a"] & SEEN and not by[b"a\x00\x00"] & SEEN
        assert by[b"1234567"] & SEEN and by[b"12345678"] & SEEN and by[b"123456789"] & SEEN
        assert not any(by[p] & SEEN for p in pads[3:]) and not by[prefixes[1]] & SEEN and by[prefixes[2]] & SEEN
        assert all(w & SEEN for w in words[len(first) + len(second):])                   # everything was added


def test_the_fold_belongs_to_the_set(core):
    pairs = []
    for a, b in ((0xC0, 0xE0), (0xC4, 0xE4), (0x81, 0xA1), (0x9A, 0xBA), (0x40, 0x60), (0x5B, 0x7B), (0x5E, 0x7E), (0x00, 0x20)):   # 0x20 apart, no letters
        pairs.append((b"k" + bytes([a]) + b"z", b"K" + bytes([b]) + b"Z", b"k" + bytes([a]) + b"Z"))
    first = [b"abc", b"MiXed"] + [p[0] for p in pairs]
    second = [b"ABC", b"mixed", b"ABC", b"new", b"new", b"abc", b"solo", b"abc"] + [x for p in pairs for x in p[1:]]
    for tag_bits in TAGS:
        words, _, dump = run_sequence(core, [(first, True), (second, True)], tag_bits=tag_bits, nocase=True)
        by = dict(zip(second, words[len(first):]))
        assert by[b"ABC"] & SEEN and by[b"mixed"] & SEEN and by[b"abc"] & SEEN and not by[b"new"] & SEEN
        for lower, other, upper in pairs:
            assert by[upper] & SEEN and not by[other] & SEEN, (lower, other)         # k<a>Z folds to k<a>z; K<b>Z is another string
        assert b"abc" in [s for _, _, s in dump] and b"ABC" not in [s for _, _, s in dump] and b"mixed" in [s for _, _, s in dump]      # the folded bytes are stored
        words, _, dump = run_sequence(core, [(first, True), (second, True)], tag_bits=tag_bits, nocase=False)
        by = dict(zip(second, words[len(first):]))
        assert not by[b"ABC"] & SEEN and not by[b"mixed"] & SEEN and by[b"abc"] & SEEN
        assert not any(by[upper] & SEEN for _, _, upper in pairs)
        assert b"ABC" in [s for _, _, s in dump] and b"MiXed" in [s for _, _, s in dump]


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_record_counts_around_a_wavefront(core, n):
    rng = random.Random(45 + n)
    held = b"held by the set"
    for n_segs in (1, 2):
        segs = []
        for _ in range(n_segs):
            seg = [text(rng, rng.randrange(1, 30), b"abcdefghij") + b"#%d" % k for k in range(n)]
            seg[0] = seg[n // 2] = seg[-1] = held                                        # the seen string first, middle and last
            if n > 3:
                seg[1] = seg[2] = b"new twice per segment"
            segs.append(seg)
        flat = [s for seg in segs for s in seg]
        m = Model()
        hs = HostSet(core, 4 * len(flat) + 4, 64 * len(flat) + 64)
        try:
            for k, (strings, cuts) in enumerate((([held, b"other"], [[held, b"other"]]), (flat, segs), (flat, segs))):
                want, want_info = m.call(strings)
                rc, got, info = hs.call(cuts, groups=1 + k, rng=rng)
                assert rc == 0 and got == want and {f: info[f] for f in want_info} == want_info, (n, k, info, want_info)
                assert sorted(s for _, _, s in hs.dump()) == sorted(m.held)
                if k == 1:
                    assert got[0] & SEEN and got[n // 2] & SEEN and got[-1] & SEEN and info["seen_distinct"] == 1
                    assert info["seen_findings"] == len([s for s in flat if s == held])
                    if n > 3:
                        decided(got + [FIRST | 1 << SHIFT])                                # (the singletons are the other records)
        finally:
            hs.free()


def snapshot(hs):
    return hs.state(), hs.dump()


def test_capacity_exactly_enough_one_string_too_few_and_eight_bytes_too_few(core):
    rng = random.Random(46)
    steps = three_results(rng, 90)
    cap_s, cap_b = capacity_of(steps)
    for tag_bits in TAGS:
        run_sequence(core, steps, None, legal_log2(cap_s), tag_bits)                      # exactly enough: succeeds, and 100 % full at the end
        for short_s, short_b in ((1, 0), (0, 8)):
            hs, m = HostSet(core, cap_s - short_s, cap_b - short_b, legal_log2(cap_s), tag_bits), Model()
            try:
                for strings, _ in steps[:2]:
                    want, _ = m.call(strings)
                    rc, got, _ = hs.call([strings])
                    assert rc == 0 and got == want
                before = snapshot(hs)
                strings = steps[2][0]
                rc, _, info = hs.call(cut(strings, 2))
                assert rc == 1, (short_s, short_b, rc)                                       # refused: what is new does not fit
                assert snapshot(hs) == before                                                # bit for bit: slots, words, entries, cursors
                assert before[0]["strings"] + info["added_strings"] == cap_s and before[0]["bytes"] + info["added_bytes"] == cap_b      # the sums the message names
                want, want_info = m.call(strings, add=False)
                rc, got, info = hs.call(cut(strings, 2), add=False)                          # the same result, lookup-only: never refused
                assert rc == 0 and got == want and {f: info[f] for f in want_info} == want_info
                decided(got)
                assert snapshot(hs) == before
            finally:
                hs.free()


def test_reset_and_the_same_result_twice(core):
    rng = random.Random(47)
    steps = three_results(rng, 80)
    first = steps[0][0]
    hs, m = HostSet(core, 1000, 40000, tag_bits=1), Model()
    try:
        for strings, _ in steps:
            want, _ = m.call(strings)
            assert hs.call([strings])[:2] == (0, want)
        decided(want)
        before = snapshot(hs)
        want, want_info = m.call(steps[2][0])
        rc, got, info = hs.call([steps[2][0]])                                               # the same result again
        assert rc == 0 and got == want and all(w & SEEN for w in got)
        assert info["added_strings"] == 0 and info["added_bytes"] == 0 and info["seen_findings"] == len(got) and info["seen_distinct"] == info["distinct"]
        assert snapshot(hs) == before
        hs.reset()
        assert hs.state()["strings"] == 0 and hs.state()["bytes"] == 0 and hs.dump() == []
        m = Model()
        want, want_info = m.call(first)
        rc, got, info = hs.call([first])
        assert rc == 0 and got == want and not any(w & SEEN for w in got) and info["seen_findings"] == 0
        assert info["added_strings"] == len(set(first)) and sorted(s for _, _, s in hs.dump()) == sorted(set(first))
    finally:
        hs.free()


def test_the_grid_changes_neither_words_nor_infos(core):
    rng = random.Random(48)
    steps = three_results(rng, 200)
    runs = [run_sequence(core, steps, (2000, 100000), -1, 1, n_segs=2, groups=g) for g in (1, 5)]
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    assert sorted(s for _, _, s in runs[0][2]) == sorted(s for _, _, s in runs[1][2])


def test_few_tag_bits_make_tags_collide_and_the_walk_compares_bytes(core):
    """(what the narrow tags are for: with 1 bit half of all pairs share a tag, with 0 bits all do)"""
    strings = sorted({text(random.Random(49), 1, b"a") + b"%d" % k for k in range(64)})
    tags = {bits: [core.sxs_seen_tag(s, len(s), 0, bits) for s in strings] for bits in TAGS}
    assert set(tags[0]) == {0} and set(tags[1]) == {0, 1} and len(set(tags[24])) > 60
    assert core.sxs_seen_home(b"MiXed", 5, 1, 10) == core.sxs_seen_home(b"mixed", 5, 1, 10)
    assert core.sxs_seen_home(b"MiXed", 5, 0, 10) != core.sxs_seen_home(b"mixed", 5, 0, 10)
