"""The keyword tally of a device-resident result (sx_tally_set_create, sx_result_tally_device): the automaton builder
(stringsext_amd/csrc/sx_seltally_build.cpp) and the tally core (sx_seltally_core.hpp) compiled as plain host C++ and driven the way
sx_seltally_dev.hip drives them (tests/native/seltally_core_host.cpp: the first lds_states rows in a place of their own, workgroups
with counters of their own for the small unique ids, rounds of one step per active lane, the flush), against Python counting by
the header's rule: hits[k] = the number of (finding, offset) pairs at which keyword k stands, first[k] = the smallest ordinal of
such a finding — after bytes.lower() of both sides for the fold, which folds 'A'..'Z' and nothing else.  The source arena ends
where a page without access begins: the core may read nothing behind the last string."""
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
NOCASE = sx.SX_SELECT_ASCII_NOCASE
NEVER = sx.SX_TALLY_NEVER
DEPS = [os.path.join(ROOT, "include", "stringsext_amd.h"), os.path.join(NATIVE, "guarded_host.hpp")] + [os.path.join(CSRC, f) for f in (
    "sx_seltally_build.cpp", "sx_seltally_build.hpp", "sx_keyword_front.hpp", "sx_seltally_core.hpp", "sx_select_core.hpp")]
LDS_ROW_BYTES, LDS_IDS = 32 * 1024, 4096      # seltally_kernel's LDS: rows and counters (sx_seltally_build.hpp)


def built(out, src, flags):
    """(as tests/test_selre_core.py builds its harness and its program: g++ on one file, rebuilt when a source is newer)"""
    out, src = os.path.join(NATIVE, out), os.path.join(NATIVE, src)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in DEPS + [src]):
        tmp = f"{out}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + ["-o", tmp, src])
        os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def core():
    L = C.CDLL(built("libseltally_core_host.so", "seltally_core_host.cpp", ["-O2", "-fPIC", "-shared"]))
    u64p, u32pp = C.POINTER(C.c_uint64), C.POINTER(C.POINTER(C.c_uint32))
    L.sxs_seltally_create.restype = C.c_void_p
    L.sxs_seltally_create.argtypes = [C.POINTER(sx.Pattern), C.c_uint32, C.c_uint32, C.POINTER(C.c_int)]
    L.sxs_seltally_free.restype, L.sxs_seltally_free.argtypes = None, [C.c_void_p]
    L.sxs_seltally_reset.restype, L.sxs_seltally_reset.argtypes = None, [C.c_void_p]
    L.sxs_seltally_info.restype, L.sxs_seltally_info.argtypes = None, [C.c_void_p, C.POINTER(sx.TallySetInfo)]
    L.sxs_seltally_tables.restype, L.sxs_seltally_tables.argtypes = None, [C.c_void_p, u32pp, u32pp, u32pp, C.POINTER(C.c_uint32)]
    L.sxs_seltally_tally.restype = C.c_int
    L.sxs_seltally_tally.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, u64p, u64p]
    L.sxs_seltally_read.restype, L.sxs_seltally_read.argtypes = C.c_int, [C.c_void_p, u64p, u64p, C.c_uint32]
    L.sxs_guarded.restype, L.sxs_guarded.argtypes = C.c_void_p, [C.c_uint64, C.POINTER(C.c_void_p), u64p]
    L.sxs_unmap.restype, L.sxs_unmap.argtypes = None, [C.c_void_p, C.c_uint64]
    return L


def fold(b, nocase):
    return b.lower() if nocase else b


def count_by_the_rule(strings, patterns, nocase=False, base=0):
    """(hits, first) per pattern, by the header's rule and nothing cleverer"""
    hits, first = [], []
    for p in patterns:
        p = fold(p, nocase)
        h, f = 0, NEVER
        for i, s in enumerate(strings):
            s = fold(s, nocase)
            c = sum(s.startswith(p, o) for o in range(len(s) - len(p) + 1))
            if c and f == NEVER:
                f = base + i
            h += c
        hits.append(h); first.append(f)
    return hits, first


def count_indexed(strings, patterns, nocase=False, base=0):
    """the same for long lists: every place of every string tried as the begin of the keywords of each length that occurs; every
    97th string is counted by the plain rule as well"""
    pats = [fold(p, nocase) for p in patterns]
    ids = {}
    for p in pats:
        ids.setdefault(p, len(ids))
    lengths = sorted({len(p) for p in ids})
    h, f = [0] * len(ids), [NEVER] * len(ids)
    for i, s in enumerate(strings):
        s = fold(s, nocase)
        here = {}
        for o in range(len(s)):
            for ln in lengths:
                if o + ln > len(s):
                    break
                k = ids.get(s[o:o + ln])
                if k is not None:
                    here[k] = here.get(k, 0) + 1
        for k, c in here.items():
            h[k] += c
            f[k] = min(f[k], base + i)
        if i % 97 == 0:
            for p, k in ids.items():            # (the rule gives 0 exactly where Python's `in` says no)
                assert (sum(s.startswith(p, o) for o in range(len(s) - len(p) + 1)) if p in s else 0) == here.get(k, 0), (i, p)
    return [h[ids[p]] for p in pats], [f[ids[p]] for p in pats]


class HostTally:
    """a set as the builder makes it; .info: sx_tally_set_info's fields; own / dict / unique_of_pattern / entries as lists"""

    def __init__(self, L, patterns, nocase=False, tables=True):
        self.L, self.patterns, self.nocase = L, [bytes(p) for p in patterns], nocase
        arr = (sx.Pattern * max(1, len(self.patterns)))(*[sx.Pattern(p, len(p)) for p in self.patterns])
        rc = C.c_int()
        self.h = L.sxs_seltally_create(arr, len(self.patterns), NOCASE if nocase else 0, C.byref(rc))
        assert rc.value == sx.SX_OK and self.h, rc.value
        i = sx.TallySetInfo()
        L.sxs_seltally_info(self.h, C.byref(i))
        self.info = info = {k: getattr(i, k) for k, _ in sx.TallySetInfo._fields_}
        # what the header promises of every set
        folded = [fold(p, nocase) for p in self.patterns]
        assert info["n_patterns"] == len(self.patterns) and info["nocase"] == int(nocase) and info["reserved"] == 0
        assert info["unique"] == len(set(folded))
        assert info["states"] == len({p[:k] for p in folded for k in range(len(p) + 1)})        # the distinct prefixes, the empty one included
        assert 1 <= info["classes"] <= 256
        assert info["entry_bytes"] == (2 if info["states"] <= 32768 else 4)
        assert info["table_bytes"] == 256 + info["states"] * info["classes"] * info["entry_bytes"] + 8 * info["states"] + 4 * len(self.patterns)
        assert info["lds_states"] == min(info["states"], LDS_ROW_BYTES // (info["classes"] * info["entry_bytes"])) >= 1
        if tables:
            own, dic, uop = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
            wide = (C.c_uint32 * (info["states"] * info["classes"]))()
            L.sxs_seltally_tables(self.h, C.byref(own), C.byref(dic), C.byref(uop), wide)
            self.own, self.dict, self.uop, self.entries = own[:info["states"]], dic[:info["states"]], uop[:len(self.patterns)], list(wide)
            self.check_tables(folded)

    def check_tables(self, folded):
        n, bit = self.info["states"], 15 if self.info["entry_bytes"] == 2 else 31
        ids = sorted(x for x in self.own if x != 0xFFFFFFFF)
        assert ids == list(range(self.info["unique"])) and self.own[0] == 0xFFFFFFFF and self.dict[0] == 0
        # equal keywords share an id, different ones do not
        assert all((self.uop[a] == self.uop[b]) == (folded[a] == folded[b]) for a in range(len(folded)) for b in range(a, min(len(folded), a + 50)))
        # a link goes to a state nearer to the root that ends a keyword; the ids grow with the state numbers (breadth first)
        assert all(d == 0 or (d < s and self.own[d] != 0xFFFFFFFF) for s, d in enumerate(self.dict))
        assert [x for x in self.own if x != 0xFFFFFFFF] == ids
        # an entry's flag says exactly "the target or its chain ends a keyword"
        for e in self.entries:
            t = e & ~(1 << bit)
            assert t < n and bool(e >> bit) == (self.own[t] != 0xFFFFFFFF or self.dict[t] != 0), (e, t)

    def chain(self, state):
        """the unique ids that end where a walk stands in `state`"""
        out = []
        while state:
            if self.own[state] != 0xFFFFFFFF:
                out.append(self.own[state])
            state = self.dict[state]
        return out

    def tally(self, strings, packed=True, layout="packed", base=0, rng=None, lds_ids=LDS_IDS, groups=2):
        """adds the strings' hits; returns (far steps, hits counted in the workgroups' counters)"""
        L = self.L
        rng = rng or random.Random(len(strings))
        offs, arena = lay_out(strings, layout, rng)
        region, region_bytes = C.c_void_p(), C.c_uint64()
        mem = L.sxs_guarded(max(1, len(arena)), C.byref(region), C.byref(region_bytes))
        assert mem
        try:
            C.memmove(mem, arena, len(arena))
            arr = records(strings, offs, packed)
            far, lds = C.c_uint64(), C.c_uint64()
            assert L.sxs_seltally_tally(self.h, C.addressof(arr), len(strings), int(packed), mem, base, lds_ids, groups, C.byref(far), C.byref(lds)) == 0
            return far.value, lds.value
        finally:
            L.sxs_unmap(region, region_bytes)

    def read(self):
        n = len(self.patterns)
        hits, first = (C.c_uint64 * n)(), (C.c_uint64 * n)()
        assert self.L.sxs_seltally_read(self.h, hits, first, n) == sx.SX_OK
        assert self.L.sxs_seltally_read(self.h, hits, first, n + 1) == sx.SX_E_INVALID
        return list(hits), list(first)

    def reset(self):
        self.L.sxs_seltally_reset(self.h)

    def free(self):
        self.L.sxs_seltally_free(self.h)
        self.h = None


def check(L, strings, patterns, nocase=False, want_hits=None, want_first=None, every=True, base=0, oracle=count_by_the_rule, **kw):
    """one set over both record types and both layouts (every=False: packed records, back to back, only), and with the counters of
    the small ids in "LDS", in HBM, and split between the two"""
    strings = list(strings)
    want = oracle(strings, patterns, nocase, base)
    if want_hits is not None:
        assert want[0] == want_hits, (want[0], want_hits)            # (the case is what its author meant)
    if want_first is not None:
        assert want[1] == want_first, (want[1], want_first)
    hs = HostTally(L, patterns, nocase)
    try:
        assert hs.read() == ([0] * len(patterns), [NEVER] * len(patterns))
        for packed in ((True, False) if every else (True,)):
            for layout in (("packed", "scattered") if every else ("packed",)):
                for lds_ids in (LDS_IDS, 0, max(1, hs.info["unique"] // 2)):
                    hs.tally(strings, packed, layout, base=base, lds_ids=lds_ids, **kw)
                    got = hs.read()
                    assert got == want, (packed, layout, lds_ids, [(p, g, w) for p, g, w in zip(patterns, zip(*got), zip(*want)) if g != w][:8])
                    hs.reset()
                    assert hs.read() == ([0] * len(patterns), [NEVER] * len(patterns))
        return want
    finally:
        hs.free()


def test_the_textbook_set_over_ushers(core):
    pats = [b"he", b"she", b"his", b"hers"]
    check(core, [b"ushers"], pats, want_hits=[1, 1, 0, 1], want_first=[0, 0, NEVER, 0])
    strings = [b"sh", b"hi", b"ushers", b"she", b"his", b"this", b"xhex", b"h", b"", b"hhhhis", b"shishers", b"sHe"]
    check(core, strings, pats, want_hits=[4, 3, 4, 2], want_first=[2, 2, 4, 2])
    check(core, strings, pats, base=1000, want_first=[1002, 1002, 1004, 1002])
    hs = HostTally(core, pats)
    assert hs.info["states"] == 10 and hs.info["unique"] == 4 and hs.info["entry_bytes"] == 2 and hs.info["lds_states"] == 10
    hs.free()


def test_overlapping_occurrences_all_count_and_the_chain_has_three_links(core):
    check(core, [b"aaaa"], [b"a", b"aa", b"aaa"], want_hits=[4, 3, 2], want_first=[0, 0, 0])
    check(core, [b"", b"a", b"aa", b"baaab", b"aaaaaaaaaa"], [b"aaa", b"a", b"aa"], want_hits=[9, 16, 12], want_first=[3, 1, 2])
    hs = HostTally(core, [b"a", b"aa", b"aaa"])
    assert hs.info["states"] == 4
    assert sorted(len(hs.chain(s)) for s in range(4)) == [0, 1, 2, 3]            # "aaa" ends three keywords: its own and two by links
    hs.free()
    check(core, [b"abababa", b"ababab", b"bab"], [b"aba", b"abab", b"bab"], want_hits=[5, 4, 5])


def test_a_suffix_a_prefix_the_whole_string_and_one_byte_keywords(core):
    strings = [b"abcdef", b"abc", b"ab", b"def", b"ef", b"f", b"xxabxx", b"cdef", b"abcde"]
    check(core, strings, [b"abcdef", b"def"], want_hits=[1, 3], want_first=[0, 0])                 # a proper suffix of another
    check(core, strings, [b"abc", b"abcdef"], want_hits=[3, 1], want_first=[0, 0])                 # a prefix: nothing is cut below its end
    check(core, strings, [b"abcdef", b"cde", b"f", b"bcdef"], want_hits=[1, 3, 5, 1], want_first=[0, 0, 0, 0])
    check(core, strings, [b"cdef", b"xxabxx", b"abcde"], want_hits=[2, 1, 2], want_first=[0, 6, 0])   # equal to a whole string
    check(core, strings, [b"f", b"x", b"q", b"a"], want_hits=[5, 4, 0, 5], want_first=[0, 6, NEVER, 0])
    check(core, [b"", b"e", b"x", b"xe", b"eee", b"E"] * 11, [b"e"], want_hits=[55], want_first=[1])
    check(core, [b"", b"e", b"x", b"xe", b"eee", b"E"] * 11, [b"e"], nocase=True, want_hits=[66])
    check(core, [b"abc"], [b"\x00"], want_hits=[0], want_first=[NEVER])


def test_bytes_above_0x7f(core):
    strings = ["Привет мир".encode(), "привет".encode(), "Добрый день".encode(), "日本語のテキスト".encode(), "テスト".encode(), b"\xd0", b"\xd1\x80",
               "naïve café".encode(), b"plain ascii", "мир".encode()[:-1], b"\xff\xff\xff"]
    check(core, strings, ["мир".encode(), "день".encode(), "テ".encode()], want_hits=[1, 1, 2], want_first=[0, 2, 3])
    check(core, strings, [b"\xd0", b"\xff\xff", b"\x80\xd0"], want_first=[0, 10, 0])
    check(core, strings, [bytes([x]) for x in range(128, 256)])
    hs = HostTally(core, [bytes([x, x]) for x in range(256)])                        # no byte is left for class 0
    assert hs.info["classes"] == 256 and hs.info["states"] == 513
    hs.free()


def test_duplicates_and_patterns_equal_only_after_the_fold(core):
    strings = [b"xx", b"ab AB aB", b"Ab", b"abab"]
    check(core, strings, [b"ab", b"ab", b"AB", b"ab"], want_hits=[3, 3, 1, 3], want_first=[1, 1, 1, 1])
    check(core, strings, [b"ab", b"AB", b"aB", b"Ab", b"b"], nocase=True, want_hits=[6, 6, 6, 6, 6], want_first=[1] * 5)
    a, b = HostTally(core, [b"Ab", b"aB", b"AB"], nocase=True), HostTally(core, [b"Ab", b"aB", b"AB"])
    assert (a.info["unique"], a.info["states"], a.info["classes"]) == (1, 3, 3)
    assert (b.info["unique"], b.info["states"], b.info["classes"]) == (3, 6, 5)
    a.free(); b.free()
    # the fold takes 'A'..'Z' and nothing else
    strings = ["Ärger".encode(), "ärger".encode(), "ÄRGER".encode(), b"[rger", b"{RGER", b"@Z`z"]
    check(core, strings, ["ärGER".encode(), b"[RGER", b"@z`Z", b"RGER"], nocase=True, want_hits=[1, 1, 1, 5], want_first=[1, 3, 5, 0])


def test_a_keyword_that_exists_only_across_two_records_counts_nothing(core):
    strings = [b"....ab", b"cd....", b"a", b"b", b"c", b"d", b"", b"abc", b"", b"d"]
    assert b"abcd" in b"".join(strings)
    check(core, strings, [b"abcd", b"bc"], want_hits=[0, 1], want_first=[NEVER, 7])
    strings = [b"0123456789"] * 63 + [b"....ab", b"cd....", b"tail"]            # at a wavefront's edge: records 63 and 64
    check(core, strings, [b"abcd", b"ab", b"cd"], want_hits=[0, 1, 1], want_first=[NEVER, 63, 64])
    rng = random.Random(9)
    strings = [text(rng, rng.randrange(4, 20), b"abcdefghijklmnopqrstuvwxyz") for _ in range(150)]
    spans = [strings[i][-3:] + strings[i + 1][:3] for i in range(149)]
    spans = [p for p in spans if not any(p in s for s in strings)]
    assert len(spans) > 100
    check(core, strings, spans, want_hits=[0] * len(spans), every=False)


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_record_counts_around_a_wavefront(core, n, packed):
    rng = random.Random(60 + n)
    strings = [text(rng, rng.randrange(0, 24), b"abc") for _ in range(n)]
    strings[-1] = b"the last one"
    pats = [b"ab", b"last one", b"cca", b"e", b"#"]
    want = count_by_the_rule(strings, pats, base=7)
    assert want[1][1] == 7 + n - 1 and want[0][4] == 0
    hs = HostTally(core, pats)
    for layout in ("packed", "scattered"):
        for groups in (1, 2, 5):
            hs.tally(strings, packed, layout, base=7, rng=rng, groups=groups)
            assert hs.read() == want
            hs.reset()
    hs.free()


def test_calls_accumulate_with_their_ordinal_base_and_reset_forgets(core):
    rng = random.Random(17)
    one = [text(rng, rng.randrange(0, 30), b"abc") for _ in range(100)]
    two = [text(rng, rng.randrange(0, 30), b"abc") for _ in range(77)] + [b"zz"]
    pats = [b"abc", b"cc", b"bab", b"zz", b"q"]
    assert not any(b"zz" in s for s in one)
    hs = HostTally(core, pats)
    hs.tally(one, base=0)
    assert hs.read() == count_by_the_rule(one, pats)
    hs.tally(two, packed=False, layout="scattered", base=len(one))                   # the second buffer of a stream
    assert hs.read() == count_by_the_rule(one + two, pats)
    assert hs.read()[1][3] == 177 and hs.read()[1][4] == NEVER
    hs.tally(one, base=len(one) + len(two))                                          # the same strings again: the hits add, first stays
    h1, h2 = count_by_the_rule(one, pats)[0], count_by_the_rule(one + two, pats)
    assert hs.read() == ([a + b for a, b in zip(h1, h2[0])], h2[1])
    hs.reset()
    assert hs.read() == ([0] * 5, [NEVER] * 5)
    hs.tally(two, base=1000)
    assert hs.read() == count_by_the_rule(two, pats, base=1000)
    hs.tally(one, base=0)                                                            # a smaller ordinal later still wins
    assert hs.read()[1][:3] == count_by_the_rule(one, pats)[1][:3]
    hs.free()


def test_6000_keywords_take_wide_entries_and_walk_rows_on_both_sides(core):
    """random 8-byte keywords over 36 letters share few prefixes — all 36 and 1296 of one and two bytes, then nearly none —: 6000 of
    them have some 37 000 states, above the 32 768 that 15 bits number, the first 5000 some 31 000"""
    rng = random.Random(5000)
    alphabet = b"abcdefghijklmnopqrstuvwxyz0123456789"
    pats = [text(rng, 8, alphabet) for _ in range(6000)]
    hs = HostTally(core, pats, tables=False)
    print(hs.info)
    assert hs.info["states"] > 32768 and hs.info["entry_bytes"] == 4 and 0 < hs.info["lds_states"] < hs.info["states"]
    assert hs.info["unique"] > LDS_IDS                                              # ids on both sides of the LDS counters' bound
    strings = [text(rng, rng.randrange(0, 40), alphabet) for _ in range(300)]
    for k in range(0, 300, 2):
        p = pats[k * 31 % 6000]
        at = rng.randrange(0, len(strings[k]) + 1)
        strings[k] = strings[k][:at] + p + p[-3:] + strings[k][at:]
    want = count_indexed(strings, pats)
    assert sum(1 for h in want[0] if h) >= 150
    for packed, layout in ((True, "packed"), (False, "scattered")):
        far, lds = hs.tally(strings, packed, layout, rng=rng)
        assert far > 0 and 0 < lds < sum(want[0])
        assert hs.read() == want
        hs.reset()
    hs.free()
    # just below the switch: 2-byte entries and rows outside LDS all the same
    narrow = HostTally(core, pats[:5000], tables=False)
    assert 20000 < narrow.info["states"] <= 32768 and narrow.info["entry_bytes"] == 2 and narrow.info["lds_states"] < narrow.info["states"]
    far, _ = narrow.tally(strings, rng=rng)
    assert far > 0 and narrow.read() == count_indexed(strings, pats[:5000])
    narrow.free()


@pytest.mark.parametrize("seed", range(30))
def test_random_cases_over_small_alphabets(core, seed):
    """2 or 3 letters: deep failure chains, dense overlaps"""
    rng = random.Random(7000 + seed)
    alphabet = rng.choice((b"ab", b"abc", b"aAb"))
    nocase = alphabet == b"aAb"
    strings = [text(rng, rng.randrange(0, 81), alphabet) for _ in range(rng.choice((300, 1000, 3000)))]
    pats = [text(rng, rng.randrange(1, 7), alphabet) for _ in range(rng.choice((1, 5, 40, 300)))]
    hs = HostTally(core, pats, nocase)
    want = count_indexed(strings, pats, nocase, base=seed)
    if seed % 5 == 0:
        assert count_indexed(strings, pats[:8], nocase, base=seed) == count_by_the_rule(strings, pats[:8], nocase, base=seed)
    half = len(strings) // 2
    hs.tally(strings[:half], seed % 2 == 0, "packed" if seed % 3 else "scattered", base=seed, rng=rng, lds_ids=rng.choice((0, 3, LDS_IDS)), groups=rng.choice((1, 3)))
    hs.tally(strings[half:], seed % 2 == 1, "scattered" if seed % 3 else "packed", base=seed + half, rng=rng, lds_ids=rng.choice((0, 3, LDS_IDS)))
    got = hs.read()
    assert got == want, [(p, g, w) for p, g, w in zip(pats, zip(*got), zip(*want)) if g != w][:8]
    hs.free()


def test_random_cases_with_wide_entries(core):
    """the same over a set with more than 32768 states: the short keywords' states lie in LDS, the long ones' do not"""
    rng = random.Random(8000)
    long_ones = [text(rng, 8, b"abcdefghijklmnopqrstuvwxyz0123456789") for _ in range(6000)]
    for seed in range(3):
        short = [text(rng, rng.randrange(1, 7), b"abc") for _ in range(200)]
        pats = short + long_ones
        rng.shuffle(pats)
        strings = [text(rng, rng.randrange(0, 81), b"abc") + rng.choice((b"", rng.choice(long_ones), rng.choice(long_ones)[:7])) for _ in range(1500)]
        hs = HostTally(core, pats, tables=False)
        assert hs.info["entry_bytes"] == 4
        far, lds = hs.tally(strings, seed % 2 == 0, "scattered", rng=rng)
        assert far > 0 and lds > 0
        assert hs.read() == count_indexed(strings, pats)
        hs.free()


def create_rc(L, pats, n=None, flags=0):
    arr = (sx.Pattern * max(1, len(pats)))(*[sx.Pattern(p, ln) for p, ln in pats])
    rc = C.c_int(99)
    h = L.sxs_seltally_create(arr, len(pats) if n is None else n, flags, C.byref(rc))
    if h:
        L.sxs_seltally_free(h)
    assert bool(h) == (rc.value == sx.SX_OK)
    return rc.value


def test_the_builders_limits_are_the_pattern_sets(core):
    L, ok, bad = core, sx.SX_OK, sx.SX_E_INVALID
    assert create_rc(L, [(b"a", 1)], n=0) == bad
    assert create_rc(L, [(b"a", 1)]) == ok
    many = [(b"ab", 2)] * 65537
    assert create_rc(L, many, n=65536) == ok
    assert create_rc(L, many, n=65537) == bad
    long_one = b"q" * 256
    assert create_rc(L, [(long_one, 0)]) == bad
    assert create_rc(L, [(long_one, 255)]) == ok
    assert create_rc(L, [(long_one, 256)]) == bad
    full = [(long_one, 255)] * 4112                                                  # 1 MiB - 16
    assert create_rc(L, full + [(long_one, 16)]) == ok
    assert create_rc(L, full + [(long_one, 17)]) == bad
    assert create_rc(L, [(None, 3)]) == bad
    rc = C.c_int(99)
    assert L.sxs_seltally_create(None, 1, 0, C.byref(rc)) is None and rc.value == bad
    assert create_rc(L, [(b"a", 1)], flags=NOCASE) == ok
    assert create_rc(L, [(b"a", 1)], flags=sx.SX_SELECT_INVERT) == bad
    assert create_rc(L, [(b"a", 1)], flags=NOCASE | 1 << 31) == bad


def test_a_sanitizer_build_counts_the_same(tmp_path):
    """the builder and the core under the address and undefined-behaviour sanitizers, as a program of their own"""
    exe = built("seltally_build_main", "seltally_build_main.cpp", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    rng = random.Random(300)
    cases = []          # (patterns, flags, lds_ids, strings, want: a code or True)
    for pats in ([b""], [b"q" * 256], [b"ok", b""]):
        cases.append((pats, 0, 0, [b"a"], sx.SX_E_INVALID))
    cases.append(([b"a"], 2, 0, [b"a"], sx.SX_E_INVALID))
    cases.append(([b"he", b"she", b"his", b"hers"], 0, LDS_IDS, [b"ushers"], True))
    cases.append(([b"a", b"aa", b"aaa"], 0, 1, [b"aaaa"], True))
    cases.append(([b"ab", b"AB", b"aB", b"ab"], NOCASE, 0, [b"xx", b"ab AB aB", b"", b"Ab"], True))
    cases.append(([b"abcd", b"bc"], 0, LDS_IDS, [b"....ab", b"cd....", b"", b"abc"], True))
    cases.append(([bytes([x]) for x in range(256)], 0, 100, [bytes(range(256)), b"\xff" * 70], True))
    cases.append(([text(rng, 8, b"abcdefghijklmnopqrstuvwxyz0123456789") for _ in range(6000)], 0, LDS_IDS, [text(rng, 60, b"abcdefgh") for _ in range(70)], True))
    for _ in range(60):
        alphabet = rng.choice((b"ab", b"abc", b"aAb"))
        strings = [text(rng, rng.randrange(0, 81), alphabet) for _ in range(rng.choice((1, 63, 64, 65, 130)))]
        pats = [text(rng, rng.randrange(1, 7), alphabet) for _ in range(rng.randrange(1, 60))]
        cases.append((pats, NOCASE if alphabet == b"aAb" else 0, rng.choice((0, 2, LDS_IDS)), strings, True))
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for pats, flags, lds_ids, strings, _ in cases:
            f.write("case %d %d\n" % (flags, lds_ids))
            f.writelines("p %s\n" % p.hex() for p in pats)
            f.writelines("s %s\n" % s.hex() for s in strings)
            f.write("end\n")
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-3000:]
    lines = run.stdout.splitlines()
    at = 0
    for pats, flags, lds_ids, strings, want in cases:
        if want is not True:
            assert lines[at].startswith("rc %d " % want), (pats, lines[at])
            at += 1
            continue
        # the program walks the strings twice, with the ordinals 100.. and 100 + n..
        hits, first = count_indexed(strings, pats, bool(flags & NOCASE), base=100)
        assert lines[at].split() == ["hits"] + [str(2 * h) for h in hits], (pats[:5], flags, lines[at][:200])
        assert lines[at + 1].split() == ["first"] + [str(f) for f in first], (pats[:5], flags, lines[at + 1][:200])
        at += 2
    assert at == len(lines)
