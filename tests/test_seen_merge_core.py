"""A seen set's merge (sx_seen_set_merge, _grow, _import, _add_strings): the lane functions (stringsext_amd/csrc/
sx_seen_merge_core.hpp) compiled as plain host C++ and driven the way sx_seen_merge_dev.hip and the entry points drive them
(tests/native/seen_merge_host.cpp: mark over the source's words, the host's look at the cursors and the totals, add), with Python sets
of (folded) byte strings as the model and sources built by hand in Python.  No expected value comes from the code under test.  Every
slot table, word list and arena ends where a page without access begins.  The harness takes table_log2 and tag_bits as they are:
tables of 2 and 4 slots make every probe a chain, tag_bits 0 and 1 make the tags collide."""
import ctypes as C
import os
import random
import re
import struct
import subprocess

import pytest

import test_seen_core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "stringsext_amd", "csrc")
DEPS = [os.path.join(ROOT, "include", "stringsext_amd.h")] + [os.path.join(NATIVE, f) for f in (
    "seen_core_host.cpp", "distinct_core_host.cpp", "seen_set_host.hpp", "guarded_host.hpp")] + [os.path.join(CSRC, f) for f in (
    "sx_seen_merge_core.hpp", "sx_seen_core.hpp", "sx_distinct_core.hpp", "sx_select_core.hpp", "sx_seltally_core.hpp")]
EMPTY = (1 << 64) - 1             # kSeenEmpty
OFFSET_BITS = 40                  # kSeenOffsetBits
SEED = 0x5EE25E70                 # kSeenSeed
M64 = (1 << 64) - 1
TAGS = (0, 1, 24)
INFO = ("source_strings", "already_held", "added_strings", "added_bytes")

# lengths 0, 1, 7, 8, 9, 15, 16, 17 and 300; pairs that differ only in the last byte, only in length (a prefix, and a NUL where the
# other's padding is), and only in a byte of the last partial word
STEM = b"0123456789abcdefXYZ"
POOL = [b"", b"a", b"seven77", b"eight888", b"nine99999", b"fifteen15151515", b"sixteen161616161", b"seventeen17171717", bytes(range(33, 133)) * 3,
        STEM[:16] + b"p", STEM[:16] + b"q",                      # 17 bytes: the last byte, alone in its word
        b"eight88", b"eight8888",                                # a prefix of, and one longer than, eight888: they differ only in length
        b"a\x00", b"a\x00\x00", b"seven77\x00",                  # ... where the shorter one's padding is
        STEM[:8] + b"abc", STEM[:8] + b"aXc", STEM[:8] + b"Xbc",  # 11 bytes: a byte of the last partial word
        b"MiXed Case", b"mixed case", b"MIXED CASE", b"k\xc0z", b"k\xe0z", b"K\xc0Z"]
assert {len(s) for s in POOL} >= {0, 1, 7, 8, 9, 15, 16, 17, 300} and len(set(POOL)) == len(POOL)


def fold(s):
    """'A'..'Z' -> 'a'..'z', no other byte"""
    return bytes(b | 0x20 if 65 <= b <= 90 else b for b in s)


def entry_bytes(n):
    """SX_SEEN_ENTRY_BYTES"""
    return 8 + (n + 7) // 8 * 8


def legal_log2(capacity_strings):
    """the power of two >= 2 x capacity_strings, at least 2 slots"""
    return next(p for p in range(1, 64) if 1 << p >= 2 * capacity_strings)


def mix(h):
    h ^= h >> 33; h = h * 0xff51afd7ed558ccd & M64
    h ^= h >> 33; h = h * 0xc4ceb9fe1a85ec53 & M64
    return h ^ h >> 33


def py_hash(s, nocase):
    """distinct_hash(s, len, nocase, kSeenSeed) of sx_distinct_core.hpp, written again"""
    h = mix((0xcbf29ce484222325 + (SEED + 1) * 0x9e3779b97f4a7c15) & M64)
    for b in (fold(s) if nocase else s):
        h = (h ^ b) * 0x100000001b3 & M64
    return mix(h ^ len(s) << 32)


def source(strings, rng=None, empties=0, high_bits=False):
    """(words, arena) for pairwise different strings: their entries in a shuffled order, the words in another; empties: that many
    kSeenEmpty words per entry strewn in, as a slot table has them; high_bits: tags of any value above the offsets"""
    rng = rng or random.Random(len(strings))
    assert len(set(strings)) == len(strings)
    order = list(strings)
    rng.shuffle(order)
    arena, at_of = b"", {}
    for s in order:
        at_of[s] = len(arena)
        arena += struct.pack("<II", len(s), 0) + s + bytes(-len(s) % 8)
    words = [at_of[s] // 8 | ((rng.getrandbits(24) << OFFSET_BITS) if high_bits else 0) for s in strings]
    words += [EMPTY] * (empties * max(1, len(strings)))
    rng.shuffle(words)
    return words, arena


@pytest.fixture(scope="module")
def core():
    out, src = os.path.join(NATIVE, "libseen_merge_host.so"), os.path.join(NATIVE, "seen_merge_host.cpp")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in DEPS + [src]):
        tmp = f"{out}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O2", "-fPIC", "-shared", "-o", tmp, src])
        os.replace(tmp, out)
    L = C.CDLL(out)
    u64p, vp = C.POINTER(C.c_uint64), C.c_void_p
    L.sxs_seen_new.restype, L.sxs_seen_new.argtypes = vp, [C.c_int32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64]
    L.sxs_seen_free.restype, L.sxs_seen_free.argtypes = None, [vp]
    L.sxs_seen_state.restype, L.sxs_seen_state.argtypes = None, [vp, u64p]
    L.sxs_seen_raw.restype, L.sxs_seen_raw.argtypes = None, [vp, u64p, C.c_char_p]
    L.sxs_seen_dump.restype, L.sxs_seen_dump.argtypes = C.c_uint64, [vp, u64p, u64p, u64p, C.c_uint64, C.c_char_p, C.c_uint64]
    L.sxm_list_new.restype, L.sxm_list_new.argtypes = vp, [u64p, C.c_uint64, C.c_char_p, C.c_uint64]
    L.sxm_list_free.restype, L.sxm_list_free.argtypes = None, [vp]
    L.sxm_hash_bytes.restype, L.sxm_hash_bytes.argtypes = C.c_uint64, [C.c_char_p, C.c_uint32, C.c_uint32]
    L.sxm_hash_entry.restype, L.sxm_hash_entry.argtypes = C.c_uint64, [C.c_char_p, C.c_uint32, C.c_uint32]
    L.sxm_merge_list.restype, L.sxm_merge_list.argtypes = C.c_int, [vp, vp, C.c_uint32, C.c_uint32, u64p, u64p]
    L.sxm_merge_set.restype, L.sxm_merge_set.argtypes = C.c_int, [vp, vp, C.c_uint32, C.c_uint32, u64p, u64p]
    # the result path's call on the same set (seen_core_host.cpp is in this library)
    vpp = C.POINTER(C.c_void_p)
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

    def state(self):
        out = (C.c_uint64 * 6)()
        self.L.sxs_seen_state(self.h, out)
        return dict(zip(("strings", "bytes", "capacity_strings", "capacity_bytes", "table_log2", "tag_bits"), out))

    def raw(self):
        """the set's memory as it lies: (cursors, slots, arena)"""
        st = self.state()
        slots, arena = (C.c_uint64 * (1 << st["table_log2"]))(), C.create_string_buffer(max(1, st["capacity_bytes"]))
        self.L.sxs_seen_raw(self.h, slots, arena)
        return (st["strings"], st["bytes"]), list(slots), arena.raw[:st["capacity_bytes"]]

    def dump(self):
        """[(slot, word, the stored string)] by a walk over the table"""
        st = self.state()
        cap = 1 << st["table_log2"]
        slot, word, ln = (C.c_uint64 * cap)(), (C.c_uint64 * cap)(), (C.c_uint64 * cap)()
        buf = C.create_string_buffer(st["bytes"] + 8)
        n = self.L.sxs_seen_dump(self.h, slot, word, ln, cap, buf, st["bytes"] + 8)
        assert n <= cap, "an entry that does not fit what the cursor says, or whose second word is not 0"
        out, at = [], 0
        for k in range(n):
            padded = (ln[k] + 7) // 8 * 8
            assert buf.raw[at + ln[k]:at + padded] == bytes(padded - ln[k]), "padding that is not 0"
            out.append((slot[k], word[k], buf.raw[at:at + ln[k]]))
            at += padded
        return out

    call = test_seen_core.HostSet.call      # the result path's call (distinct, mark, add) on this very set: (code, words, info)

    def merge(self, src, add=True, groups=2):
        """src: a HostSet (its slot table is the source) or (words, arena); (the harness's code, info as a dict, held per source word)"""
        L = self.L
        info = (C.c_uint64 * 4)()
        if isinstance(src, HostSet):
            n = 1 << src.state()["table_log2"]
            held = (C.c_uint64 * ((n + 63) // 64))()
            rc = L.sxm_merge_set(self.h, src.h, groups, int(not add), held, info)
        else:
            words, arena = src
            n = len(words)
            held = (C.c_uint64 * max(1, (n + 63) // 64))(*([0xEEEEEEEEEEEEEEEE] * max(1, (n + 63) // 64)))
            lst = L.sxm_list_new((C.c_uint64 * max(1, n))(*words), n, arena, len(arena))
            assert lst
            try:
                rc = L.sxm_merge_list(self.h, lst, groups, int(not add), held, info)
            finally:
                L.sxm_list_free(lst)
        return rc, dict(zip(INFO, info)), [bool(held[i // 64] >> (i % 64) & 1) for i in range(n)]


def want_info(held, src, add=True):
    new = src - held
    return dict(source_strings=len(src), already_held=len(src & held), added_strings=len(new) if add else 0, added_bytes=sum(entry_bytes(len(s)) for s in new) if add else 0)


def check(hs, model):
    """the destination's contents — a walk over its table — and its cursors against the model"""
    st, dump = hs.state(), hs.dump()
    assert sorted(s for _, _, s in dump) == sorted(model), (sorted(s for _, _, s in dump), sorted(model))
    assert len({w & (1 << OFFSET_BITS) - 1 for _, w, _ in dump}) == len(dump)              # every slot its own entry
    assert (st["strings"], st["bytes"]) == (len(model), sum(entry_bytes(len(s)) for s in model)), st


def merge_and_check(hs, model, src_strings, add=True, groups=2, rng=None, empties=0, high_bits=False):
    """one call with a hand-built source against the model (a Python set, updated); returns the info"""
    strings = sorted(src_strings)
    words, arena = source(strings, rng, empties, high_bits)
    rc, info, held = hs.merge((words, arena), add, groups)
    assert rc == 0, rc
    assert info == want_info(model, set(strings), add), (info, want_info(model, set(strings), add))
    by_offset = {}
    o = 0
    while o < len(arena):
        n = int.from_bytes(arena[o:o + 4], "little")
        by_offset[o // 8] = arena[o + 8:o + 8 + n]
        o += entry_bytes(n)
    for w, h in zip(words, held):                                                        # held[] per source word, empties never
        assert h == (w != EMPTY and by_offset[w & (1 << OFFSET_BITS) - 1] in model), (hex(w), h)
    if add:
        model |= set(strings)
    check(hs, model)
    return info


def cases(pool, room):
    """(name, the destination's strings, the source's) with a union of `room` strings at most; what does not fit `room` is left out"""
    half = max(1, min(len(pool) // 2, (room + 1) // 2))
    a, b = pool[:half], pool[half:2 * half]
    out = [("empty source", a[:room], []), ("empty destination", [], a[:room]), ("identical", a[:room], a[:room]), ("both empty", [], [])]
    if room >= 2:
        n = min(room, len(a + b))
        out += [("disjoint", a[:room // 2], b[:room // 2]), ("subset", a[:room], a[:room:2]), ("superset", a[:room:2], a[:room]),
                ("overlap", (a + b)[:n - 1], (a + b)[1:n])]
    return out


@pytest.mark.parametrize("nocase", [False, True])
@pytest.mark.parametrize("tag_bits", TAGS)
@pytest.mark.parametrize("table_log2", [1, 2, None])
def test_merges_against_python_sets(core, table_log2, tag_bits, nocase):
    """(a table the harness is told to make has 2^table_log2 - 1 strings at most: one slot stays empty, so every probe ends)"""
    rng = random.Random(100 + tag_bits)
    pool = sorted({fold(s) for s in POOL}) if nocase else list(POOL)
    rng.shuffle(pool)
    room = len(pool) if table_log2 is None else (1 << table_log2) - 1
    seen_cases = set()
    for name, dst, src in cases(pool, room):
        for empties, high_bits in ((0, False), (2, True)):                    # a dense list; a slot table with empties and tags
            union = set(dst) | set(src)
            cap_s, cap_b = max(1, len(union)), sum(entry_bytes(len(s)) for s in union)
            hs = HostSet(core, cap_s, cap_b, legal_log2(cap_s) if table_log2 is None else table_log2, tag_bits, nocase)
            try:
                model = set()
                merge_and_check(hs, model, dst, rng=rng, groups=1)                                  # (into the empty set)
                before = hs.raw()
                merge_and_check(hs, model, src, add=False, rng=rng, empties=empties, high_bits=high_bits)
                assert hs.raw() == before                                                           # a lookup writes nothing
                info = merge_and_check(hs, model, src, rng=rng, empties=empties, high_bits=high_bits, groups=3)
                assert model == union
                if cap_b:
                    st = hs.state()
                    assert (st["strings"], st["bytes"]) == (len(union), cap_b)                      # filled to the last byte
                again = merge_and_check(hs, model, src, rng=rng, empties=empties)                   # the same again: all held
                assert again["added_strings"] == 0 and again["already_held"] == len(set(src))
                seen_cases.add((name, info["added_strings"] > 0, info["already_held"] > 0))
            finally:
                hs.free()
    assert ("identical", False, True) in seen_cases and ("empty destination", True, False) in seen_cases
    if room >= 2:
        assert ("disjoint", True, False) in seen_cases and ("overlap", True, True) in seen_cases and ("subset", False, True) in seen_cases


@pytest.mark.parametrize("nocase", [False, True])
@pytest.mark.parametrize("tag_bits", TAGS)
@pytest.mark.parametrize("table_log2", [1, 2, None])
def test_the_result_path_and_the_merge_path_agree_about_one_set(core, table_log2, tag_bits, nocase):
    """What the result path's add put into a set, the merge path's lookup finds — held[] bit for bit over a list source of POOL —, and
    what the merge path's add put into a set, a following result call marks SX_DISTINCT_SEEN: exactly the model's strings, the model
    being a Python set."""
    rng = random.Random(300 + tag_bits)
    key = fold if nocase else (lambda s: s)
    pool = sorted({key(s) for s in POOL})                                    # what a source may hold: pairwise different, folded
    room = len(pool) - 4 if table_log2 is None else (1 << table_log2) - 1     # (some of POOL stay outside: held[] and SEEN have both values)
    findings = list(POOL) + rng.sample(POOL, 9)                              # a result: every string, some twice, unfolded
    rng.shuffle(findings)
    put, model = [], set()                                                   # the findings a result call adds: `room` classes
    for s in findings:
        if key(s) in model or len(model) < room:
            put.append(s)
            model.add(key(s))
    assert len(model) == room
    cap_b = sum(entry_bytes(len(s)) for s in model)
    log2 = legal_log2(room) if table_log2 is None else table_log2
    # the result path fills, the merge path looks up
    hs = HostSet(core, room, cap_b, log2, tag_bits, nocase)
    try:
        rc, _, info = hs.call([put], rng=rng)
        assert rc == 0 and info["added_strings"] == room, (rc, info)
        check(hs, model)
        merge_and_check(hs, model, pool, add=False, rng=rng)                 # held[] per source word against the model, info, nothing written
        merge_and_check(hs, model, pool, add=False, rng=rng, empties=2, high_bits=True, groups=3)
    finally:
        hs.free()
    # the merge path fills, the result path looks up
    hs = HostSet(core, room, cap_b, log2, tag_bits, nocase)
    try:
        merge_and_check(hs, set(), model, rng=rng)
        m = test_seen_core.Model(nocase)
        m.held = set(model)
        want, want_info = m.call(findings, add=False)
        rc, got, info = hs.call([findings], add=False, rng=rng)
        assert rc == 0 and got == want, [(s, hex(g), hex(w)) for s, g, w in zip(findings, got, want) if g != w][:5]
        assert {f: info[f] for f in want_info} == want_info
        assert [bool(w & test_seen_core.SEEN) for w in got] == [key(s) in model for s in findings]
        assert any(key(s) in model for s in findings) and any(key(s) not in model for s in findings)
        check(hs, model)
    finally:
        hs.free()


@pytest.mark.parametrize("nocase", [False, True])
@pytest.mark.parametrize("tag_bits", TAGS)
def test_a_sets_slot_table_as_the_source_and_growth(core, tag_bits, nocase):
    """set -> set, as sx_seen_set_merge and sx_seen_set_grow run it: the source's table as it lies, most of it empty"""
    rng = random.Random(7 + tag_bits)
    pool = sorted({fold(s) for s in POOL}) if nocase else list(POOL)
    more = [b"w%d" % k for k in range(300)]
    a, b = set(pool[:14]) | set(more[:150]), set(pool[7:]) | set(more[100:])
    assert a & b and a - b and b - a
    cap = lambda strs, extra=0: (len(strs) + extra, sum(entry_bytes(len(s)) for s in strs) + 16 * extra)
    src, dst = HostSet(core, *cap(b, 40), tag_bits=tag_bits, nocase=nocase), HostSet(core, *cap(a | b), tag_bits=tag_bits, nocase=nocase)
    grown = HostSet(core, *cap(a | b, 700), tag_bits=tag_bits, nocase=nocase)
    small = HostSet(core, *cap(a | b), table_log2=legal_log2(len(a | b)), tag_bits=1, nocase=nocase)
    try:
        ms, md = set(), set()
        merge_and_check(src, ms, b, rng=rng)
        merge_and_check(dst, md, a, rng=rng)
        before_src = src.raw()
        rc, info, _ = dst.merge(src, add=False)
        assert rc == 0 and info == want_info(md, ms, add=False)
        check(dst, md)
        rc, info, _ = dst.merge(src, groups=3)
        assert rc == 0 and info == want_info(md, ms)
        md |= ms
        check(dst, md)
        assert src.raw() == before_src                                                               # the source is only read
        st = dst.state()
        assert (st["strings"], st["bytes"]) == (st["capacity_strings"], st["capacity_bytes"])
        # growth: everything into an empty, larger set whose table has another size — and into one with other tag bits
        for other in (grown, small):
            rc, info, _ = other.merge(dst, groups=1)
            assert rc == 0 and info == want_info(set(), md)
            check(other, md)
        assert grown.state()["table_log2"] > dst.state()["table_log2"]
        rc, info, _ = dst.merge(grown)                                                               # back: all held, nothing written
        assert rc == 0 and info == want_info(md, md)
    finally:
        for hs in (src, dst, grown, small):
            hs.free()


@pytest.mark.parametrize("tag_bits", TAGS)
def test_capacity_one_string_short_and_one_byte_short_leaves_the_destination_bit_for_bit(core, tag_bits):
    rng = random.Random(11)
    have, new = set(POOL[:10]), set(POOL[6:])
    union = have | new
    cap_s, cap_b = len(union), sum(entry_bytes(len(s)) for s in union)
    for short_s, short_b in ((0, 0), (1, 0), (0, 1), (0, 8)):
        hs = HostSet(core, cap_s - short_s, cap_b - short_b, legal_log2(cap_s), tag_bits)
        try:
            model = set()
            merge_and_check(hs, model, have, rng=rng)
            before = hs.raw()
            words, arena = source(sorted(new), rng, empties=1)
            rc, info, _ = hs.merge((words, arena), groups=2)
            if not short_s and not short_b:
                assert rc == 0 and hs.raw() != before
                continue
            assert rc == 1, (short_s, short_b, rc)                                                   # refused: what is new does not fit
            assert hs.raw() == before                                                                # bit for bit: cursors, slots, entries
            assert info == want_info(model, new)                                                     # the sums the message names
            assert before[0][0] + info["added_strings"] == cap_s and before[0][1] + info["added_bytes"] == cap_b
            rc, info, _ = hs.merge((words, arena), add=False)                                        # lookup-only: never refused
            assert rc == 0 and info == want_info(model, new, add=False) and hs.raw() == before
        finally:
            hs.free()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_word_counts_around_a_wavefront_and_a_grid_that_strides(core, n):
    strings = [b"s%d" % k + b"x" * (k % 11) for k in range(n)]
    held_first = {strings[0], strings[n // 2], strings[-1]}
    for groups in (1, 2):
        hs = HostSet(core, 2 * n + 2, 64 * n + 64, tag_bits=1)
        try:
            model = set()
            merge_and_check(hs, model, held_first, groups=groups)
            info = merge_and_check(hs, model, strings, groups=groups, rng=random.Random(n))
            assert info["already_held"] == len(held_first) and info["added_strings"] == n - len(held_first)
        finally:
            hs.free()
    # more words than one trip of either pass's grid: 1 group x 8 wavefronts x 64 words (mark), x kSeenMergeAddChunks (add), then one more
    chunks = int(re.search(r"constexpr\s+uint32_t\s+kSeenMergeAddChunks\s*=\s*(\d+)", open(os.path.join(CSRC, "sx_seen_merge_core.hpp")).read()).group(1))
    many = [b"m%d" % k for k in range(8 * 64 * chunks + 1)]
    hs = HostSet(core, len(many), 16 * len(many))
    try:
        model = set()
        merge_and_check(hs, model, many[::3], groups=1)
        merge_and_check(hs, model, many, groups=1, empties=1)
    finally:
        hs.free()


def test_a_probe_that_wraps_and_a_full_table_raises_the_error(core):
    """(a table told to be full: the harness's capacity lets the host pass, the kernels' bounded walks must say so)"""
    hs = HostSet(core, 4, 256, table_log2=1, tag_bits=0)
    try:
        model = set()
        merge_and_check(hs, model, [b"one"])
        rc, _, _ = hs.merge(source([b"two"]))                                                        # fills the second of two slots
        assert rc == 0
        rc, _, _ = hs.merge(source([b"three"]), add=False)                                           # no empty slot: the lookup's walk ends
        assert rc == -3
        rc, _, _ = hs.merge(source([b"one"]), add=False)                                             # what is there is still found
        assert rc == 0
    finally:
        hs.free()


@pytest.mark.parametrize("nocase", [0, 1])
def test_the_word_wise_hash_is_distinct_hash(core, nocase):
    rng = random.Random(5 + nocase)
    for n in range(0, 41):
        for _ in range(4):
            s = bytes(rng.choice(b"AZaz@[`{\x00\xff\xc1\xe1mM09") if rng.random() < 0.6 else rng.randrange(256) for _ in range(n))
            if nocase:
                assert core.sxm_hash_bytes(s, n, 1) == py_hash(s, True)                              # of raw bytes, which it folds
                s = fold(s)                                                                          # (an entry holds folded bytes)
            want = py_hash(s, bool(nocase))
            assert core.sxm_hash_entry(s, n, nocase) == want == core.sxm_hash_bytes(s, n, nocase), (n, s)
    s = bytes(rng.randrange(256) for _ in range(300))
    assert core.sxm_hash_entry(s, 300, 0) == py_hash(s, False)
