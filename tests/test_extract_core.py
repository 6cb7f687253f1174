"""The extraction of regex matches (sx_extract_regex_create, sx_result_extract_regex_device): the extract builder
(stringsext_amd/csrc/sx_extract_build.cpp) and the lane functions (sx_extract_core.hpp) compiled as plain host C++ and driven the way
sx_extract_dev.hip drives them (tests/native/extract_core_host.cpp: the first rows in a place of their own, wavefront after wavefront
rounds of one step per active lane, the per-record counts, the scan, pass 2 from the stored counts, the ordered gather), against a
brute force over Python's `re`: at offset o the largest e in (o, n] such that some pattern, followed by exactly n - e more bytes and
the end, matches at o — `^` stays at the real start, `$` at the real end, laziness decides nothing.  The expected value never comes
from the code under test.  The source arena ends where a page without access begins."""
import ctypes as C
import functools
import hashlib
import os
import random
import re
import subprocess
import time

import pytest

import stringsext_amd as sx
from test_select_core import lay_out, records, text
from test_selre_core import DEEP, PINNED_SETS, REFUSED, Tree, to_python

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "stringsext_amd", "csrc")
NOCASE = sx.SX_SELECT_ASCII_NOCASE
DEPS = [os.path.join(ROOT, "include", "stringsext_amd.h"), os.path.join(NATIVE, "guarded_host.hpp")] + [os.path.join(CSRC, f) for f in (
    "sx_extract_build.cpp", "sx_extract_build.hpp", "sx_extract_core.hpp", "sx_selre_front.hpp", "sx_selset_build.hpp", "sx_select_core.hpp", "sx_result_core.hpp")]


def built(out, src, flags):
    """(as tests/test_selre_core.py builds its harness: g++ on one file, rebuilt when a source is newer)"""
    out, src = os.path.join(NATIVE, out), os.path.join(NATIVE, src)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in DEPS + [src]):
        tmp = f"{out}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + flags + ["-o", tmp, src])
        os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def core():
    L = C.CDLL(built("libextract_core_host.so", "extract_core_host.cpp", ["-O2", "-fPIC", "-shared"]))
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    L.sxs_extract_create.restype = C.c_void_p
    L.sxs_extract_create.argtypes = [C.POINTER(sx.Pattern), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.c_char_p, C.c_uint32]
    L.sxs_extract_free.restype, L.sxs_extract_free.argtypes = None, [C.c_void_p]
    L.sxs_extract_info.restype, L.sxs_extract_info.argtypes = None, [C.c_void_p, C.POINTER(sx.ExtractRegexInfo), u32p]
    L.sxs_extract_table.restype, L.sxs_extract_table.argtypes = C.c_uint64, [C.c_void_p, C.c_void_p, C.c_uint64]
    L.sxs_extract_host.restype = C.c_int
    L.sxs_extract_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, u32p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                   u64p, u64p, u64p, u64p]
    L.sxs_guarded.restype, L.sxs_guarded.argtypes = C.c_void_p, [C.c_uint64, C.POINTER(C.c_void_p), u64p]
    L.sxs_unmap.restype, L.sxs_unmap.argtypes = None, [C.c_void_p, C.c_uint64]
    return L


# ---- the oracle

@functools.lru_cache(maxsize=None)
def ends_at(p, k, nocase):
    return re.compile(b"(?:" + to_python(p) + b")(?s:.{%d})\\Z" % k, re.IGNORECASE if nocase else 0)


def matches(patterns, nocase, s):
    """the (o, e) of s as grep -oE finds them: leftmost start, longest end over all patterns, no overlap, none empty"""
    out, o, n = [], 0, len(s)
    while o < n:
        e = next((e for e in range(n, o, -1) if any(ends_at(p, n - e, nocase).match(s, o) for p in patterns)), None)
        if e is None:
            o += 1
        else:
            out.append((o, e)); o = e
    return out


def test_the_oracle_is_what_the_issue_says():
    assert matches([rb"[0-9]+\.[0-9]+"], False, b"ip 10.0.0.1 and 3.14") == [(3, 7), (8, 11), (16, 20)]
    assert matches([b"^ab|b+"], False, b"abbbab") == [(0, 2), (2, 4), (5, 6)]
    assert matches([b"a*"], False, b"baab") == [(1, 3)]


# ---- the harness

def create(L, pats, n=None, flags=0, lds_cap=0):
    """(handle or None, extract_build's code, its text) for (bytes, len) pairs"""
    arr = (sx.Pattern * max(1, len(pats)))(*[sx.Pattern(p, ln) for p, ln in pats])
    rc, err = C.c_int(99), C.create_string_buffer(512)
    h = L.sxs_extract_create(arr, len(pats) if n is None else n, flags, lds_cap, C.byref(rc), err, 512)
    assert bool(h) == (rc.value == sx.SX_OK)
    return h, rc.value, err.value.decode(errors="replace")


def create_rc(L, pats, n=None, flags=0):
    h, rc, err = create(L, pats, n, flags)
    if h:
        L.sxs_extract_free(h)
    return rc, err


class HostExtract:
    """a set as the builder makes it; .info: sx_extract_regex_info's fields plus end_first, here_first, dead_first, start0, start1"""

    def __init__(self, L, patterns, nocase=False, lds_cap=0):
        self.L, self.patterns, self.nocase, self.lds_cap = L, [bytes(p) for p in patterns], nocase, lds_cap
        self.h, rc, err = create(L, [(p, len(p)) for p in self.patterns], flags=NOCASE if nocase else 0, lds_cap=lds_cap)
        assert rc == sx.SX_OK and self.h, (rc, err, self.patterns)
        i, shape = sx.ExtractRegexInfo(), (C.c_uint32 * 5)()
        L.sxs_extract_info(self.h, C.byref(i), shape)
        self.info = dict({k: getattr(i, k) for k, _ in sx.ExtractRegexInfo._fields_},
                         end_first=shape[0], here_first=shape[1], dead_first=shape[2], start0=shape[3], start1=shape[4])
        f = self.info      # what the header and sx_extract_build.hpp promise of every set
        assert f["n_patterns"] == len(self.patterns) and f["nocase"] == int(nocase)
        assert 1 <= f["classes"] <= 256 and 1 <= f["states"] <= sx.SX_SELECT_REGEX_MAX_STATES
        assert f["table_bytes"] == f["states"] * f["classes"] * 2
        assert f["lds_states"] == min(f["states"], 48 * 1024 // (f["classes"] * 2))
        assert f["end_first"] <= f["here_first"] <= f["dead_first"] <= f["states"] <= f["dead_first"] + 1
        assert f["start0"] < f["states"] and f["start1"] < f["states"]

    def table(self):
        buf = C.create_string_buffer(40 + 256 + self.info["table_bytes"])
        n = self.L.sxs_extract_table(self.h, buf, len(buf))
        assert n == len(buf)
        return buf.raw

    def free(self):
        self.L.sxs_extract_free(self.h)
        self.h = None


def rest(r, packed):
    """every field of a record but str_off and str_len"""
    return (r.position, r.flags, r.mission_id) if packed else \
        (r.position, r.precision, r.completes_previous, r.mission_id, r.reserved, r.input_file_id, r.reserved2, r.slice_index)


def check_set(L, hx, strings, packed=True, layout="packed", rng=None, want=None, expect=None):
    """hx over `strings` laid out as `layout`, against the oracle (expect: what it has said of them already); returns (the matches
    per string, steps outside "LDS", all steps)"""
    rng = rng or random.Random(len(strings))
    strings = list(strings)
    offs, arena = lay_out(strings, layout, rng)
    n = len(strings)
    region, region_bytes = C.c_void_p(), C.c_uint64()
    base = L.sxs_guarded(max(1, len(arena)), C.byref(region), C.byref(region_bytes))
    assert base
    try:
        C.memmove(base, arena, len(arena))
        arr = records(strings, offs, packed)
        expect = expect or [matches(hx.patterns, hx.nocase, s) for s in strings]
        if want is not None:
            assert expect == list(want), (hx.patterns, expect, want)     # (the case is what its author meant)
        flat = [(i, o, e) for i, ms in enumerate(expect) for o, e in ms]
        total = sum(e - o for _, o, e in flat)
        assert total <= sum(len(s) for s in strings)
        out = ((sx.Finding16 if packed else sx.Finding) * max(1, len(flat)))()
        raw = C.create_string_buffer(b"\xEE" * (total + 64), total + 64)
        counts = (C.c_uint32 * max(1, n))()
        n_out, out_bytes, far_steps, steps = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        rc = L.sxs_extract_host(hx.h, C.addressof(arr), n, int(packed), base, counts, C.addressof(out), len(flat), C.addressof(raw), total,
                                C.byref(n_out), C.byref(out_bytes), C.byref(far_steps), C.byref(steps))
        assert rc == 0, (rc, hx.patterns, n_out.value, len(flat), out_bytes.value, total)
        if n:
            assert list(counts[:n]) == [len(ms) for ms in expect], (hx.patterns, hx.nocase, [(strings[i], expect[i], counts[i]) for i in range(n) if counts[i] != len(expect[i])][:5])
        assert (n_out.value, out_bytes.value) == (len(flat), total)
        out_arena = raw.raw
        assert out_arena[total:] == b"\xEE" * 64, "bytes behind the matches were written"
        off = 0
        for k, (i, o, e) in enumerate(flat):
            assert rest(out[k], packed) == rest(arr[i], packed), (k, i)           # the finding's record, unchanged but for
            assert (out[k].str_off, out[k].str_len) == (off, e - o), (k, i, o, e, out[k].str_off, out[k].str_len)   # back to back, in order
            assert out_arena[off:off + e - o] == strings[i][o:e], (k, i, o, e)
            off += e - o
        assert off == total
        return expect, far_steps.value, steps.value
    finally:
        L.sxs_unmap(region, region_bytes)


def check(L, strings, patterns, nocase=False, want=None, every=True, **kw):
    """one set over both record types and both layouts (every=False: packed records, back to back, only)"""
    if isinstance(patterns, bytes):
        patterns = [patterns]
    hx = HostExtract(L, patterns, nocase)
    try:
        expect = None
        for packed in ((True, False) if every else (True,)):
            for layout in (("packed", "scattered") if every else ("packed",)):
                expect, _, _ = check_set(L, hx, strings, packed, layout, want=want, **kw)
        return expect
    finally:
        hx.free()


# ---- 1. hand-written cases

def test_the_issues_three_examples(core):
    check(core, [b"ip 10.0.0.1 and 3.14"], rb"[0-9]+\.[0-9]+", want=[[(3, 7), (8, 11), (16, 20)]])
    check(core, [b"abbbab"], b"^ab|b+", want=[[(0, 2), (2, 4), (5, 6)]])
    check(core, [b"baab"], b"a*", want=[[(1, 3)]])


def test_leftmost_longest_not_leftmost_first(core):
    check(core, [b"abcabc", b"ab", b"xabcx", b"a"], b"a|ab|abc", want=[[(0, 3), (3, 6)], [(0, 2)], [(1, 4)], [(0, 1)]])
    check(core, [b"abcabc", b"ab", b"xabcx", b"a"], [b"a", b"ab", b"abc"], want=[[(0, 3), (3, 6)], [(0, 2)], [(1, 4)], [(0, 1)]])   # alternatives from different patterns
    check(core, [b"abcabc"], [b"abc", b"a"], want=[[(0, 3), (3, 6)]])
    check(core, [b"abcd abd"], [b"ab", b"abcd", b"bd"], want=[[(0, 4), (5, 7)]])       # bd is overlapped by the earlier ab
    check(core, [b"aaaa"], b"aa", want=[[(0, 2), (2, 4)]])
    check(core, [b"aaa"], b"aa", want=[[(0, 2)]])
    check(core, [b"xaaay"], b"a+?", want=[[(1, 4)]])                                    # lazy: accepted and ignored
    check(core, [b"xaaay"], b"a{1,2}?", want=[[(1, 3), (3, 4)]])
    check(core, [b"foobar foo"], b"foo(bar)?", want=[[(0, 6), (7, 10)]])
    check(core, [b"abab"], b"(ab)*c|a", want=[[(0, 1), (2, 3)]])                        # a walk that runs on and falls back to an early end


def test_anchors_hold_at_the_strings_own_ends_for_every_match(core):
    check(core, [b"aaa", b"baa", b"a", b""], b"^a", want=[[(0, 1)], [], [(0, 1)], []])
    check(core, [b"aaa", b"aab", b"a", b""], b"a$", want=[[(2, 3)], [], [(0, 1)], []])
    check(core, [b"aaa"], b"^a|a$", want=[[(0, 1), (2, 3)]])
    check(core, [b"abab", b"ab", b"xab"], b"^ab$", want=[[], [(0, 2)], []])
    check(core, [b"abcabc"], b"^abc|c", want=[[(0, 3), (5, 6)]])
    check(core, [b"abcabc"], b"abc$|a", want=[[(0, 1), (3, 6)]])
    check(core, [b"xx"], b"(^|x)x", want=[[(0, 2)]])
    check(core, [b"xxx"], b"(^|x)x", want=[[(0, 2)]])              # the third x has no x in front of it that is not taken
    check(core, [b"xxxx"], b"x(x|$)", want=[[(0, 2), (2, 4)]])
    check(core, [b"xxx"], b"x(x|$)", want=[[(0, 2), (2, 3)]])
    check(core, [b"ab\n", b"ab", b"\nab"], b"ab$", want=[[], [(0, 2)], [(1, 3)]])      # no "in front of a trailing newline" rule
    check(core, [b"ab"], b"a^b|b$a", want=[[]])


def test_a_dollar_never_looks_into_the_next_records_bytes(core):
    # back to back: "....ab" is followed by "c...", "ab" by the inaccessible page
    strings = [b"....ab", b"c...", b"ab", b"", b"b", b"ab"]
    check(core, strings, b"ab$", want=[[(4, 6)], [], [(0, 2)], [], [], [(0, 2)]])
    check(core, strings, b"abc", want=[[], [], [], [], [], []])           # only across two strings: nowhere
    check(core, strings, b"^c|^b", want=[[], [(0, 1)], [], [], [(0, 1)], []])
    check(core, strings, b"b.", want=[[], [], [], [], [], []])
    check(core, strings, b"ab(c|$)", want=[[(4, 6)], [], [(0, 2)], [], [], [(0, 2)]])


def test_empty_matches_are_never_emitted(core):
    strings = [b"", b"baab", b"xyz", b"a", b""]
    check(core, strings, b"a*", want=[[], [(1, 3)], [], [(0, 1)], []])
    check(core, strings, b"x?", want=[[], [], [(0, 1)], [], []])
    check(core, strings, b"^", want=[[], [], [], [], []])
    check(core, strings, b"$", want=[[], [], [], [], []])
    check(core, strings, b"^$", want=[[], [], [], [], []])
    check(core, strings, b"()", want=[[], [], [], [], []])
    check(core, strings, b"|b", want=[[], [(0, 1), (3, 4)], [], [], []])
    check(core, [b""] * 65, b"^$|a*", want=[[]] * 65)


def test_the_fold_and_bytes_from_0x80(core):
    strings = [b"MiXeD mixed MIXED", b"[`_", "Ärger ärger".encode(), b"\xc3\x84\xc3\xa4", b"\xff\xfe\x80"]
    check(core, strings, b"mixed", nocase=True, want=[[(0, 5), (6, 11), (12, 17)], [], [], [], []])
    check(core, strings, b"mixed", want=[[(6, 11)], [], [], [], []])
    check(core, strings, b"[Z-a]+", nocase=True, want=[[], [(0, 3)], [], [], []])
    check(core, [b"mzAaZm[M"], b"[Z-a]+", nocase=True, want=[[(1, 5), (6, 7)]])                    # a class holds a letter's other case too
    check(core, [b"mzAaZm[M"], b"[Z-a]+", want=[[(3, 5), (6, 7)]])
    check(core, strings, b"\xc3\x84", nocase=True, want=[[], [], [(0, 2)], [(0, 2)], []])        # no byte >= 0x80 is folded
    check(core, strings, b"\xc3[\x84\xa4]", want=[[], [], [(0, 2), (7, 9)], [(0, 2), (2, 4)], []])
    check(core, strings, "ä+".encode(), want=[[], [], [(7, 9)], [(2, 4)], []])                    # C3 A4+: the + binds A4 alone
    check(core, strings, rb"[\x80-\xff]+", want=[[], [], [(0, 2), (7, 9)], [(0, 4)], [(0, 3)]])
    check(core, strings, rb"\xfe.", want=[[], [], [], [], [(1, 3)]])


def test_matches_that_touch_and_a_match_that_is_the_whole_string(core):
    check(core, [b"123", b"1a23", b""], b"[0-9]", want=[[(0, 1), (1, 2), (2, 3)], [(0, 1), (2, 3), (3, 4)], []])
    check(core, [b"abab", b"ab"], b"ab", want=[[(0, 2), (2, 4)], [(0, 2)]])
    check(core, [b"hello world", b"x"], b".*", want=[[(0, 11)], [(0, 1)]])
    check(core, [b"hello world"], b"^hello world$", want=[[(0, 11)]])
    check(core, [b"a\nb"], b".+", want=[[(0, 1), (2, 3)]])
    check(core, [b"k" * 300], b"k{255}", want=[[(0, 255)]])
    check(core, [b"k" * 300], b"k+", want=[[(0, 300)]], every=False)
    s = b"user@example.com, other@host.org; http://a.b/c?d=e 10.1.2.3"
    check(core, [s], [rb"[a-z0-9.]+@[a-z0-9.]+\.[a-z]+", rb"https?://[^ ]+", rb"([0-9]{1,3}\.){3}[0-9]{1,3}"],
          want=[[(0, 16), (18, 32), (34, 50), (51, 59)]])


# ---- 2. the edges of a wavefront, both record types, both layouts

@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_record_counts_around_a_wavefront(core, n, packed):
    rng = random.Random(170 + n)
    strings = [text(rng, rng.randrange(0, 24), b"abc ") for _ in range(n)]
    strings[-1] = b"ab the last one ab"
    if n >= 65:
        strings[62:65] = [b"ab..ab", b"....ab", b"cab..."]      # records 63 and 64: a wavefront's last and the next one's first
    some, none, every = HostExtract(core, [b"ab+c?|^c", b"one$|ab$"]), HostExtract(core, [b"#"]), HostExtract(core, [b"[^#]"])
    for layout in ("packed", "scattered"):
        expect, _, _ = check_set(core, some, strings, packed, layout, rng=rng)
        if n != 65:
            assert expect[-1] == [(0, 2), (16, 18)]           # `one` is not at the end
        assert any(len(ms) >= 2 for ms in expect) and any(not ms for ms in expect[:-1] or [[]])
        if n >= 65:
            assert expect[63] == [(4, 6)] and expect[64] == [(0, 1), (1, 3)]      # ....ab is followed by c, and takes none of it
        check_set(core, none, strings, packed, layout, rng=rng, want=[[]] * n)                                  # the empty result
        check_set(core, every, strings, packed, layout, rng=rng, want=[[(k, k + 1) for k in range(len(s))] for s in strings])   # a record per byte
    for hx in (some, none, every):
        hx.free()


def test_rows_in_lds_and_rows_in_the_table(core):
    rng = random.Random(4800)
    words = [text(rng, 8, b"abcdefghijklmnopqrstuvwxyz") for _ in range(60)]
    pats = [b"|".join(words[k:k + 20]) for k in range(0, 60, 20)]
    strings = [text(rng, rng.randrange(0, 48), b"abcdefghijklmnopqrstuvwxyz") for _ in range(200)]
    for k in range(0, 200, 2):
        at = rng.randrange(0, len(strings[k]) + 1)
        strings[k] = strings[k][:at] + words[k * 7 % 60][:rng.choice((8, 8, 7))] + strings[k][at:] + words[k % 60]
    results = []
    for lds_cap in (0, 3, 1):      # what the builder allows; the two starts and one row; one row
        hx = HostExtract(core, pats, lds_cap=lds_cap)
        assert hx.info["states"] > 100
        for packed, layout in ((True, "packed"), (False, "scattered")):
            expect, far, steps = check_set(core, hx, strings, packed, layout, rng=rng)
            assert (far > 0) == (lds_cap != 0) and steps > 0, (lds_cap, far)
            results.append(expect)
        hx.free()
    assert all(r == results[0] for r in results) and sum(len(ms) for ms in results[0]) >= 100


# ---- 3. random cases

ALPHABET = b"abcdef\n"


def backtracks(node, inside=False):
    """a repeat or an alternation inside an unbounded repeat: the oracle's engine may take exponential time to say no"""
    kind = node[0]
    if kind == "rep":
        return inside or backtracks(node[5], inside or node[1] in ("*", "+", "{m,}"))
    if kind in ("cat", "alt"):
        return inside and kind == "alt" or any(backtracks(k, inside) for k in node[1])
    return kind == "group" and backtracks(node[2], inside)


def random_tree(rng):
    while True:
        t = Tree(rng, ALPHABET if rng.random() < 0.8 else b"abAB_ 9\n", rng.randrange(0, 5))
        if not backtracks(t.node):
            return t


def random_case(rng):
    """(patterns, nocase, strings): strings of at most 48 bytes over six letters and the newline"""
    trees = [random_tree(rng) for _ in range(rng.choice((1, 1, 1, 2, 3)))]
    pats = [t.render() for t in trees]
    assert all(1 <= len(p) <= 1024 for p in pats)
    strings = []
    for _ in range(rng.choice((1, 2, 5, 9))):
        r = rng.random()
        s = text(rng, rng.randrange(0, rng.choice((5, 12, 24, 49))), ALPHABET)
        if r < 0.5:
            m = rng.choice(trees).sample()
            at = rng.randrange(len(s) + 1)
            s = s[:at] + m + s[at:]
            if r < 0.2:
                s += rng.choice(trees).sample()
        strings.append(s[:48])
    return pats, rng.random() < 0.3, strings


def test_2000_random_cases(core):
    rng = random.Random(2000)
    cases = [random_case(rng) for _ in range(2000)]
    # what the oracle says of the cases, before anything is compared: they decide something
    expects = []
    for pats, nocase, strings in cases:
        expects.append([matches(pats, nocase, s) for s in strings])
        ends_at.cache_clear()
    with_match = sum(any(e) for e in expects)
    with_two = sum(any(len(ms) >= 2 for ms in e) for e in expects)
    assert with_match * 3 >= len(cases) and with_two * 10 >= len(cases) and (len(cases) - with_match) * 10 >= len(cases), (with_match, with_two)
    for (pats, nocase, strings), expect in zip(cases, expects):
        hx = HostExtract(core, pats, nocase, lds_cap=rng.choice((0, 0, 1, 2, 5)))      # (a refused case fails here: the generator stays inside the language and the limits)
        try:
            check_set(core, hx, strings, rng.random() < 0.5, rng.choice(("packed", "scattered")), rng=rng, expect=expect)
        finally:
            hx.free()


# ---- 4. the builder

def test_equivalent_patterns_give_the_same_table(core):
    def table(p, nocase=False):
        hx = HostExtract(core, [p] if isinstance(p, bytes) else p, nocase)
        t = hx.table()
        hx.free()
        return t[4:]      # (but for n_patterns)
    for group in ((b"a+", b"aa*", b"a{1,}", b"a+?", b"(a|aa)+", b"a|aa|a{3,}"),
                  (b"colou?r", b"color|colour", b"colo(?:u|)r", [b"color", b"colour"], [b"colour", b"color", b"color"]),
                  (b"x{2,3}", b"xxx?", b"xx|xxx", [b"xxx", b"xx"]),
                  (b"^a|b$", b"b$|^a", [b"^a", b"b$"], b"(?:^a)|(?:b$)"),
                  (b"[0-9]+", rb"\d+", rb"\d\d*", b"[0-9]{1,}"),
                  (b"a*", b"a+", b"(a*)*", b"a*|a")):          # the empty match is never taken: what differs only in it is the same
        tables = [table(p) for p in group]
        assert all(t == tables[0] for t in tables), group
    assert table(b"Ab", nocase=True) == table(b"aB|AB|ab", nocase=True) != table(b"Ab")
    assert table(b"ab") != table(b"ab$") != table(b"^ab")
    # the shape of a small one: `ab` — start, a, ab (here), dead; two starts that coincide; a, b, every other byte
    hx = HostExtract(core, [b"ab"])
    f = hx.info
    assert (f["states"], f["classes"], f["end_first"], f["here_first"], f["dead_first"], f["start0"], f["start1"]) == (4, 3, 2, 2, 3, 0, 0), f
    hx.free()
    hx = HostExtract(core, [b"^ab$"])
    f = hx.info      # start0, a, ab (end), dead = start1
    assert (f["states"], f["end_first"], f["here_first"], f["dead_first"], f["start0"], f["start1"]) == (4, 2, 3, 3, 0, 3), f
    hx.free()


def test_every_refused_form_and_limit_is_the_regex_sets_with_the_same_text(core):
    import test_selre_core as selre
    R = C.CDLL(selre.built("libselre_core_host.so", "selre_core_host.cpp", ["-O2", "-fPIC", "-shared"]))
    R.sxs_selre_create.restype = C.c_void_p
    R.sxs_selre_create.argtypes = [C.POINTER(sx.Pattern), C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.c_char_p, C.c_uint32]
    R.sxs_selre_free.restype, R.sxs_selre_free.argtypes = None, [C.c_void_p]
    bad = sx.SX_E_INVALID
    long_one = b"q" * 1025
    lists = [([(p, len(p))], None, 0) for p, _ in REFUSED] + [([(b"ok", 2), (b"a|b", 3), (p, len(p))], None, NOCASE) for p, _ in REFUSED[::5]]
    lists += [([(p, len(p))], None, 0) for p, compiles in DEEP if not compiles]
    lists += [([(b"ab", 2)] * 65, 0, 0), ([(b"ab", 2)] * 65, 65, 0), ([(long_one, 0)], None, 0), ([(b"ok", 2), (long_one, 1025)], None, 0),
              ([(None, 3)], None, 0), ([(b"a", 1)], None, sx.SX_SELECT_INVERT), ([(b"a", 1)], None, 4), ([(b"a", 1)], None, NOCASE | 1 << 31),
              ([(b"a{256}", 6)], None, 0), ([(b"a{3,2}", 6)], None, 0), ([(b"((a{255}){255}){255}", 20)], None, 0), ([(b"(((){255}){255}){255}", 21)], None, 0),
              ([(b"^(a{255}){200}", 14)] * 2, None, 0), ([(b"^[ab]*a[ab]{16}$", 16)], None, 0)]
    for pats, n, flags in lists:
        rc, err = create_rc(core, pats, n, flags)
        h, rc2, err2 = selre.create(R, pats, n, flags)
        assert h is None and rc == rc2 == bad and err == err2 and err, (pats[-1][0][:30], rc, rc2, err, err2)
    for p, off in REFUSED:
        rc, err = create_rc(core, [(p, len(p))])
        assert "pattern 0, offset %d:" % off in err, (p, err)
    for p in (b"a{255}", b"a{0,255}", b"}", b"]", b"a|", b"|", b"()", b"(|)", b"\\{1\\}", b"[{]", b"a{,3}", b"-", b"[a-]", b"(?:)", b"a*?", b"a+?", b"a??", b"a{2,3}?"):
        rc, err = create_rc(core, [(p, len(p))])
        assert rc == sx.SX_OK, (p, err)
    assert create_rc(core, [(b"ab", 2)] * 64)[0] == sx.SX_OK and create_rc(core, [(long_one, 1024)])[0] == sx.SX_OK
    rc, err = C.c_int(99), C.create_string_buffer(64)
    assert core.sxs_extract_create(None, 1, 0, 0, C.byref(rc), err, 64) is None and rc.value == bad
    # the states: an anchored walk needs 2^15 of them here as well, and 2^17 are refused
    hx = HostExtract(core, [b"^[ab]*a[ab]{14}$"])
    assert 2 ** 15 <= hx.info["states"] <= 2 ** 15 + 2 and hx.info["classes"] == 3
    check_set(core, hx, [b"a" + b"b" * 14, b"ba" + b"a" * 14, b"b" * 15, b"xa" + b"b" * 14],
              want=[[(0, 15)], [(0, 16)], [], []])
    hx.free()
    for p, compiles in DEEP:
        if compiles:
            t0 = time.perf_counter()
            rc, err = create_rc(core, [(p, len(p))])
            assert rc == sx.SX_OK and time.perf_counter() - t0 < 1.0, (p[:20], err)


# sha256 of sxs_extract_table's bytes — ten words of ExtractTable, the class map, the entries — of test_selre_core.PINNED_SETS, in
# its order, as commit 046f17a gave them, the last one in which extract_build had a subset construction, a numbering and a row
# writer of its own: its output has not changed by a bit
EXTRACT_PINNED = [
    "a2c7a946d01ab59951395ac3650cdbd16b31a7602b51cba2eece0d6c7478c103", "998c78a2e52bb590b0bb2406938e4422e66b35de18adbee2dc0dfa846bb038b6",
    "84803aa2d76f083d603b3de893bc5e4ad2024dd2594a518efdb8c49cfca7aab3", "1080ef1262d92abd94671de15ef363667e5d1fc826c6270c9a6c1068aaa2b764",
    "4284f52226c0028295a954bead6282f1dc0847e1db85bf66d6576679b2f9dd28", "fce2b6e726ae66015be8a810a503e2e311d3a0c6073bb9d4b1487fd92f26b59f",
    "5098b76a0dbf99ec310084b55824e487d11ad095b91c54853216f5b233a58f56", "131a16aa129fe3f4c3ba36d19be850632c9c45aa5b051cee7bde2c1686418f74",
    "d1d2a9225228288c55f4251f57cfc932b0506bac7ef1b8baa6ea4884b15ac4bb", "e4b60262073c764435e3ca95d0b86ae886493b46949c78fa49456b821f751159",
    "e4b60262073c764435e3ca95d0b86ae886493b46949c78fa49456b821f751159", "201ce1a9fa3930b0e75486ad3a5856c34f175363c1a5b1996fa280d863f275f3",
    "64587c2551a5aaea32e0154a596df51c0bec5bcb495bf8be5ef3cee8162bffe7", "be22078bb6ddc962e1bec352188d4b421c876076922e139e79b2b4c8b2e928e6",
    "c9ad4493767e3bf0dba37cfca9a7ac92ef5c19a606f8c88aaf3c2c9f8c610aa5", "af3109e5c6bb91dea650b2374b282b497b04b45b74cd2d20f4c5318d3d86dcfb",
    "efc363fde00caff2c6347c829cdec6631a68535fbecca69a8f5f2715a1d5bb23",
]


def test_the_extract_sets_tables_are_unchanged(core):
    assert len(EXTRACT_PINNED) == len(PINNED_SETS)
    shapes = set()
    for (pats, flags), digest in zip(PINNED_SETS, EXTRACT_PINNED):
        hx = HostExtract(core, pats, flags == NOCASE)
        assert hashlib.sha256(hx.table()).hexdigest() == digest, pats
        f = hx.info
        shapes.add((f["start0"] == f["start1"], f["dead_first"] < f["states"], f["end_first"] < f["here_first"], f["here_first"] < f["dead_first"]))
        hx.free()
    # every branch of the numbering is among them: one start and two, with and without `dead`, end states, here states
    assert all({True, False} <= {s[k] for s in shapes} for k in range(4)), shapes


# ---- 5. the quadratic case, loosely

def test_a_star_b_over_a_long_run_of_a_returns(core):
    hx = HostExtract(core, [b"a*b"])
    strings = [b"a" * 4096, b"aab", b"a" * 4096]
    offs, arena = lay_out(strings, "packed", random.Random(0))
    arr = records(strings, offs, False)
    out, raw, counts = (sx.Finding * 4)(), C.create_string_buffer(64), (C.c_uint32 * 3)()
    n_out, out_bytes, far, steps = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    t0 = time.perf_counter()
    rc = core.sxs_extract_host(hx.h, C.addressof(arr), 3, 0, arena, counts, C.addressof(out), 4, C.addressof(raw), 64,
                               C.byref(n_out), C.byref(out_bytes), C.byref(far), C.byref(steps))
    assert rc == 0 and list(counts) == [0, 1, 0] and (n_out.value, out_bytes.value) == (1, 3) and raw.raw[:3] == b"aab"
    assert steps.value == 2 * (4096 * 4097 // 2) + 3      # every walk runs to the end of its run of a: quadratic, as the header says
    assert time.perf_counter() - t0 < 20.0
    hx.free()


# ---- 6. the builder and the lane functions under the address and undefined-behaviour sanitizers, as a program of their own

def test_a_sanitizer_build_refuses_and_extracts_the_same(tmp_path):
    exe = built("extract_build_main", "extract_build_main.cpp", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    rng = random.Random(301)
    cases = []      # (patterns, flags, strings, want: a code or the matches)
    for p, _ in REFUSED:
        cases.append(([p], 0, [b"a"], sx.SX_E_INVALID))
    for pats in ([b"ab"] * 65, [b"q" * 1025], [b"a{256}"], [b"a{3,2}"], [b"^[ab]*a[ab]{16}$"], [b"((a{255}){255}){255}"], [b""]):
        cases.append((pats, 0, [b"a"], sx.SX_E_INVALID))
    cases.append(([b"a"], 4, [b"a"], sx.SX_E_INVALID))
    # (the oracle's engine backtracks through a hundred nested repeats for ever: it is asked what the pattern means without them)
    plain = [b"a+", b"a+", b"a*", b"a+", b"(ab)+", None, None, None, b"a"]
    assert len(plain) == len(DEEP) and all((q is not None) == compiles for q, (_, compiles) in zip(plain, DEEP))
    for (p, compiles), q in zip(DEEP, plain):
        strings = [b"", b"a", b"b", b"aaa", b"ba", b"xaby", b"abab"]
        cases.append(([p], 0, strings, [matches([q], False, s) for s in strings] if compiles else sx.SX_E_INVALID))
    for _ in range(300):
        pats, nocase, strings = random_case(rng)
        cases.append((pats, NOCASE if nocase else 0, strings, [matches(pats, nocase, s) for s in strings]))
        ends_at.cache_clear()
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for pats, flags, strings, _ in cases:
            f.write("case %d\n" % flags)
            f.writelines("p %s\n" % p.hex() for p in pats)
            f.writelines("s %s\n" % s.hex() for s in strings)
            f.write("end\n")
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-3000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases)
    for line, (pats, flags, strings, want) in zip(lines, cases):
        if isinstance(want, int):
            assert line.startswith("rc %d " % want), (pats, line)
        else:
            assert line.split() == ["m"] + ["%d:%d-%d" % (i, o, e) for i, ms in enumerate(want) for o, e in ms], (pats, flags, line, want)
