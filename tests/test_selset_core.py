"""The selection by a compiled keyword list (sx_select_set_create, sx_result_select_set_device): the automaton builder
(stringsext_amd/csrc/sx_selset_build.cpp) and the match core (sx_selset_core.hpp) compiled as plain host C++ and driven the way
sx_selset_dev.hip drives them (tests/native/selset_core_host.cpp: the first lds_states rows in a place of their own, wavefront
after wavefront rounds of one step per active lane, the ballot; then the list selection's scan, placement and ordered gather),
against Python's `any(p in s for p in patterns)` — after bytes.lower() for the fold, which folds 'A'..'Z' and nothing else.  The
source arena ends where a page without access begins: the core may read nothing behind the last string."""
import ctypes as C
import os
import random
import subprocess
import time

import pytest

import stringsext_amd as sx
from test_select_core import fields, lay_out, matches, records, text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "stringsext_amd", "csrc")
NOCASE = sx.SX_SELECT_ASCII_NOCASE


def build_selset_core():
    """(as tests/test_select_core.py builds its harness: g++ on one file, rebuilt when a source is newer)"""
    so, src = os.path.join(NATIVE, "libselset_core_host.so"), os.path.join(NATIVE, "selset_core_host.cpp")
    deps = [src, os.path.join(NATIVE, "guarded_host.hpp"), os.path.join(NATIVE, "select_pass2_host.hpp"), os.path.join(ROOT, "include", "stringsext_amd.h")] + [os.path.join(CSRC, f) for f in (
        "sx_selset_build.cpp", "sx_selset_build.hpp", "sx_keyword_front.hpp", "sx_selset_core.hpp", "sx_select_core.hpp", "sx_result_core.hpp")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", tmp, src])
        os.replace(tmp, so)
    return so


@pytest.fixture(scope="module")
def core():
    L = C.CDLL(build_selset_core())
    u64p = C.POINTER(C.c_uint64)
    L.sxs_selset_create.restype = C.c_void_p
    L.sxs_selset_create.argtypes = [C.POINTER(sx.Pattern), C.c_uint32, C.c_uint32, C.POINTER(C.c_int)]
    L.sxs_selset_free.restype, L.sxs_selset_free.argtypes = None, [C.c_void_p]
    L.sxs_selset_info.restype = None
    L.sxs_selset_info.argtypes = [C.c_void_p, C.POINTER(sx.SelectSetInfo), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.sxs_selset_select_host.restype = C.c_int
    L.sxs_selset_select_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                         C.c_uint64, u64p, u64p, u64p, u64p]
    L.sxs_guarded.restype, L.sxs_guarded.argtypes = C.c_void_p, [C.c_uint64, C.POINTER(C.c_void_p), u64p]
    L.sxs_unmap.restype, L.sxs_unmap.argtypes = None, [C.c_void_p, C.c_uint64]
    return L


class HostSet:
    """a set as the builder makes it; .info: sx_select_set_info's fields plus entry_bytes and matched"""

    def __init__(self, L, patterns, nocase=False):
        self.L, self.patterns, self.nocase = L, [bytes(p) for p in patterns], nocase
        arr = (sx.Pattern * max(1, len(self.patterns)))(*[sx.Pattern(p, len(p)) for p in self.patterns])
        rc = C.c_int()
        self.h = L.sxs_selset_create(arr, len(self.patterns), NOCASE if nocase else 0, C.byref(rc))
        assert rc.value == sx.SX_OK and self.h, rc.value
        i, eb, m = sx.SelectSetInfo(), C.c_uint32(), C.c_uint32()
        L.sxs_selset_info(self.h, C.byref(i), C.byref(eb), C.byref(m))
        self.info = dict({k: getattr(i, k) for k, _ in sx.SelectSetInfo._fields_}, entry_bytes=eb.value, matched=m.value)
        # what the header promises of every set
        assert self.info["n_patterns"] == len(self.patterns) and self.info["nocase"] == int(nocase)
        assert 1 <= self.info["classes"] <= 256
        assert 2 <= self.info["states"] <= sum(len(p) for p in self.patterns) + 2
        assert self.info["matched"] == self.info["states"] - 1
        assert self.info["entry_bytes"] == (2 if self.info["states"] <= 65536 else 4)
        assert self.info["table_bytes"] == self.info["states"] * self.info["classes"] * self.info["entry_bytes"]
        assert 1 <= self.info["lds_states"] <= self.info["states"]
        assert self.info["lds_states"] * self.info["classes"] * self.info["entry_bytes"] <= 48 * 1024

    def free(self):
        self.L.sxs_selset_free(self.h)
        self.h = None


def create_rc(L, pats, n=None, flags=0):
    """selset_build's code for (bytes, len) pairs"""
    arr = (sx.Pattern * max(1, len(pats)))(*[sx.Pattern(p, ln) for p, ln in pats])
    rc = C.c_int(99)
    h = L.sxs_selset_create(arr, len(pats) if n is None else n, flags, C.byref(rc))
    if h:
        L.sxs_selset_free(h)
    assert bool(h) == (rc.value == sx.SX_OK)
    return rc.value


def check_set(L, hs, strings, packed=True, layout="packed", invert=False, rng=None, want_selected=None):
    """hs over `strings` laid out as `layout`, against Python; returns (the selected indices, the steps outside "LDS")"""
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
        want = [i for i, s in enumerate(strings) if matches(s, hs.patterns, hs.nocase) != invert]
        if want_selected is not None:
            assert want == want_selected, (want, want_selected)     # (the case is what its author meant)
        total = sum(len(strings[i]) for i in want)
        out = ((sx.Finding16 if packed else sx.Finding) * max(1, n))()
        raw = C.create_string_buffer(b"\xEE" * (total + 64), total + 64)
        waves = (n + 63) // 64
        masks = (C.c_uint64 * (waves + 1))()
        n_sel, sel_bytes, far_steps = C.c_uint64(), C.c_uint64(), C.c_uint64()
        rc = L.sxs_selset_select_host(hs.h, C.addressof(arr), n, int(packed), base, int(invert), C.addressof(out), C.addressof(raw), total,
                                      masks, C.byref(n_sel), C.byref(sel_bytes), C.byref(far_steps))
        assert rc == 0, rc
        got = [w * 64 + b for w in range(waves) for b in range(64) if masks[w] >> b & 1] if n else []
        assert got == want, (sorted(set(got) ^ set(want))[:10], len(got), len(want))
        assert (n_sel.value, sel_bytes.value) == (len(want), total)
        out_arena = raw.raw
        assert out_arena[total:] == b"\xEE" * 64, "bytes behind the selected strings were written"
        off = 0
        for k, i in enumerate(want):
            assert fields(out[k], packed) == fields(arr[i], packed), (k, i)           # every record unchanged except str_off
            assert out[k].str_off == off, (k, out[k].str_off, off)                  # back to back, in record order
            assert out_arena[off:off + len(strings[i])] == strings[i], (k, i)
            off += len(strings[i])
        return want, far_steps.value
    finally:
        L.sxs_unmap(region, region_bytes)


def check(L, strings, patterns, nocase=False, want_selected=None, every=True, **kw):
    """one set over both record types and both layouts (every=False: packed records, back to back, only)"""
    hs = HostSet(L, patterns, nocase)
    try:
        want = None
        for packed in ((True, False) if every else (True,)):
            for layout in (("packed", "scattered") if every else ("packed",)):
                want, _ = check_set(L, hs, strings, packed, layout, want_selected=want_selected, **kw)
        return want
    finally:
        hs.free()


def test_the_textbook_set_and_a_keyword_that_ends_inside_anothers_path(core):
    pats = [b"he", b"she", b"his", b"hers"]
    strings = [b"ushers", b"she", b"sh", b"hi", b"his", b"this", b"xhex", b"h", b"e", b"s", b"ers", b"rs", b"", b"hhhhis", b"shis", b"sHe"]
    check(core, strings, pats, want_selected=[0, 1, 4, 5, 6, 13, 14])
    # "she" is walked to its end in "ushers" before "he" can show: only the failure chain of s-h-e says that "he" ends there
    check(core, [b"ushers", b"sh", b"shx", b"she"], [b"he", b"shy"], want_selected=[0, 3])
    check(core, [b"abcd", b"xbcx", b"abc", b"bc", b"b", b"abx"], [b"abcde", b"bc"], want_selected=[0, 1, 2, 3])
    check(core, [b"aabaabaac", b"aabaabaa", b"abaac"], [b"aabaac"], want_selected=[0])


def test_a_prefix_a_proper_suffix_and_a_duplicate(core):
    strings = [b"abcdef", b"abc", b"ab", b"def", b"ef", b"f", b"xxabxx", b"cdef", b"abcde"]
    check(core, strings, [b"abc", b"abcdef"], want_selected=[0, 1, 8])            # a prefix of another
    check(core, strings, [b"abcdef", b"abc"], want_selected=[0, 1, 8])            # (in the other order: below a keyword's end nothing is kept)
    check(core, strings, [b"abcdef", b"def"], want_selected=[0, 3, 7])            # a proper suffix of another
    check(core, strings, [b"abcdef", b"cde"], want_selected=[0, 7, 8])            # an infix
    check(core, strings, [b"ab", b"ab"], want_selected=[0, 1, 2, 6, 8])           # a duplicate
    check(core, strings, [b"ef", b"ab", b"ef", b"ab", b"ef"], want_selected=[0, 1, 2, 3, 4, 6, 7, 8])
    hs = HostSet(core, [b"ab", b"ab", b"ab"])
    assert hs.info["states"] == 3 and hs.info["classes"] == 3 and hs.info["n_patterns"] == 3      # root, "a", matched; class 0, a, b
    hs.free()


def test_one_pattern_of_one_byte(core):
    strings = [b"", b"e", b"x", b"xe", b"ex", b"xxxxxxxx", b"E"] * 11
    check(core, strings, [b"e"], want_selected=[i for i in range(77) if i % 7 in (1, 3, 4)])
    check(core, strings, [b"e"], nocase=True, want_selected=[i for i in range(77) if i % 7 in (1, 3, 4, 6)])
    check(core, strings, [b"\x00"], want_selected=[])


def test_a_pattern_of_255_bytes(core):
    rng = random.Random(255)
    pat = text(rng, 255, b"abc")
    strings = [b"short", pat, pat[:254], pat[1:], b"x" + pat, pat + b"x", pat[:254] + b"#", b"y" * 300 + pat + b"y" * 300, pat[:100] + pat]
    check(core, strings, [pat], want_selected=[1, 4, 5, 7, 8])
    check(core, [pat[:254]], [pat], want_selected=[])
    check(core, [pat], [pat], want_selected=[0])


def test_patterns_of_utf8_sequences(core):
    strings = ["Привет мир".encode(), "привет".encode(), "Добрый день".encode(), "日本語のテキスト".encode(), "テスト".encode(), b"\xd0", b"\xd1\x80",
               "naïve café".encode(), b"plain ascii", "мир".encode()[:-1]]
    check(core, strings, ["мир".encode(), "день".encode()], want_selected=[0, 2])
    check(core, strings, ["テ".encode()], want_selected=[3, 4])
    check(core, strings, [b"\xd0"], want_selected=[0, 1, 2, 5, 9])                # a lead byte alone is a pattern like any other
    check(core, strings, ["р".encode(), "é".encode()], want_selected=[0, 1, 2, 6, 7])   # (the cut "мир" ends with D1 alone)
    check(core, strings, [b"\x80\xd0"], want_selected=[i for i, s in enumerate(strings) if b"\x80\xd0" in s])


def test_nocase_is_compiled_into_the_set_and_folds_ascii_letters_only(core):
    strings = ["Ärger".encode(), "ärger".encode(), "ÄRGER".encode(), b"\xc3\x84RGER", b"\xc3\xa4RGER", b"[rger", b"{RGER", b"@Z`z", b"@z`Z",
               "É".encode(), "é".encode(), b"MiXeD CaSe", b"mixed case", b"MIXED CASE"]
    check(core, strings, ["Ärger".encode()], want_selected=[0])
    check(core, strings, ["Ärger".encode()], nocase=True, want_selected=[0, 2, 3])          # C3 84 is not C3 A4
    check(core, strings, ["ärGER".encode()], nocase=True, want_selected=[1, 4])
    check(core, strings, [b"[RGER"], nocase=True, want_selected=[5])                          # '[' = 'Z' + 1, '{' = 'z' + 1
    check(core, strings, [b"@Z`Z"], nocase=True, want_selected=[7, 8])                        # '@' = 'A' - 1, '`' = 'a' - 1
    check(core, strings, ["É".encode()], nocase=True, want_selected=[9])                      # C3 89 does not match C3 A9
    check(core, strings, ["é".encode()], nocase=True, want_selected=[10])
    check(core, strings, [b"mIxEd", b"CASE"], nocase=True, want_selected=[11, 12, 13])
    check(core, strings, [b"mIxEd", b"CASE"], want_selected=[13])
    check(core, strings, [b"RGER"], nocase=True, invert=True, want_selected=[7, 8, 9, 10, 11, 12, 13])
    # the fold is in the classes: the upper-case letters of a folded set are no classes of their own
    a, b = HostSet(core, [b"Ab", b"aB", b"AB"], nocase=True), HostSet(core, [b"Ab", b"aB", b"AB"])
    assert (a.info["classes"], a.info["states"]) == (3, 3) and (b.info["classes"], b.info["states"]) == (5, 4)   # root, "a" [or "A"], matched / root, "A", "a", matched
    a.free(); b.free()


def test_a_pattern_that_exists_only_across_two_records_is_selected_nowhere(core):
    strings = [b"....ab", b"cd....", b"a", b"b", b"c", b"d", b"", b"abc", b"", b"d"]
    assert b"abcd" in b"".join(strings) and not any(b"abcd" in s for s in strings)
    for packed in (True, False):
        hs = HostSet(core, [b"abcd"])
        check_set(core, hs, strings, packed, "packed", want_selected=[])
        hs.free()
    check(core, strings, [b"abcd", b"bc"], want_selected=[7])
    # at a wavefront's edge: records 63 and 64
    strings = [b"0123456789"] * 63 + [b"....ab", b"cd....", b"tail"]
    check(core, strings, [b"abcd"], want_selected=[])
    check(core, strings, [b"ab", b"cd"], want_selected=[63, 64])
    # the tail of string i and the head of string i + 1, for every i of a random text
    rng = random.Random(9)
    strings = [text(rng, rng.randrange(4, 20), b"abcdefghijklmnopqrstuvwxyz") for _ in range(150)]
    spans = [strings[i][-3:] + strings[i + 1][:3] for i in range(149)]
    spans = [p for p in spans if not any(p in s for s in strings)]
    assert len(spans) > 100
    check(core, strings, spans, want_selected=[], every=False)


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_record_counts_around_a_wavefront(core, n, packed):
    rng = random.Random(60 + n)
    strings = [text(rng, rng.randrange(0, 24), b"abc") for _ in range(n)]
    strings[-1] = b"the last one"
    hs, none = HostSet(core, [b"ab", b"last one", b"cca"]), HostSet(core, [b"#"])
    for layout in ("packed", "scattered"):
        for invert in (False, True):
            check_set(core, hs, strings, packed, layout, invert=invert, rng=rng)
        check_set(core, none, strings, packed, layout, rng=rng, want_selected=[])                          # nothing selected
        check_set(core, none, strings, packed, layout, invert=True, rng=rng, want_selected=list(range(n)))  # everything selected
    want, _ = check_set(core, hs, strings, packed)
    assert n - 1 in want
    hs.free(); none.free()


def test_invert_and_the_plain_selection_partition_the_records(core):
    rng = random.Random(40)
    strings = [text(rng, rng.randrange(0, 30), b"abc") for _ in range(700)]
    hs = HostSet(core, [b"abc", b"cc", b"bab"])
    for packed in (True, False):
        for layout in ("packed", "scattered"):
            a, _ = check_set(core, hs, strings, packed, layout, rng=rng)
            b, _ = check_set(core, hs, strings, packed, layout, invert=True, rng=rng)
            assert a and b and sorted(a + b) == list(range(700))
    hs.free()


def test_3000_patterns_walk_rows_in_lds_and_rows_in_the_table(core):
    """3000 random patterns of 3..12 bytes over a 6-letter alphabet, each drawn uniformly from ALL such strings (so most are long:
    there are 6 times as many of 12 bytes as of 11).  Drawn with uniform LENGTHS instead, some 300 of them have 3 bytes and cover
    most of the 216 possible ones: nearly every state is `matched`, under 200 are left and all lie in LDS — the second set here,
    which walks no row of the table."""
    rng = random.Random(3000)
    sizes = [6 ** ln for ln in range(3, 13)]
    pats = []
    for _ in range(3000):
        k = rng.randrange(sum(sizes))
        ln = 3
        while k >= sizes[ln - 3]:
            k -= sizes[ln - 3]; ln += 1
        pats.append(bytes(b"abcdef"[k // 6 ** j % 6] for j in range(ln)))
    assert all(3 <= len(p) <= 12 for p in pats)
    t0 = time.perf_counter()
    hs = HostSet(core, pats)
    built = time.perf_counter() - t0
    print(f"3000 patterns: {hs.info}, built in {built * 1e3:.1f} ms")
    assert hs.info["states"] > hs.info["lds_states"] and hs.info["classes"] == 7
    strings = [text(rng, rng.randrange(0, 60), b"abcdefg") for _ in range(1500)]
    for k in range(0, 1500, 3):     # (a random 12-byte pattern occurs in no random string)
        at = rng.randrange(0, len(strings[k]) + 1)
        strings[k] = strings[k][:at] + pats[k * 7 % 3000][:rng.choice((12, 12, 11, 8))] + strings[k][at:]
    for packed, layout in ((True, "packed"), (False, "scattered"), (True, "scattered"), (False, "packed")):
        want, far = check_set(core, hs, strings, packed, layout, rng=rng)
        assert 200 < len(want) < len(strings) and far > 0       # (half of the 500 insertions are whole patterns)
        check_set(core, hs, strings, packed, layout, invert=True, rng=rng)
    hs.free()
    short = HostSet(core, [text(rng, rng.randrange(3, 13), b"abcdef") for _ in range(3000)])
    assert short.info["states"] == short.info["lds_states"] < 300
    want, far = check_set(core, short, strings, rng=rng)
    assert 0 < len(want) < len(strings) and far == 0
    short.free()


def test_10000_patterns_are_built_in_milliseconds_and_more_than_65536_states_take_wide_entries(core):
    rng = random.Random(10000)
    pats = [text(rng, 12, b"abcdefghijklmnopqrstuvwxyz0123456789") for _ in range(10000)]
    t0 = time.perf_counter()
    hs = HostSet(core, pats)
    built = time.perf_counter() - t0
    print(f"10000 patterns: {hs.info}, built in {built * 1e3:.1f} ms")
    assert built < 0.5          # (seconds: a builder that did 256-wide work per state and pattern byte would not get here)
    assert hs.info["states"] > 65536 and hs.info["entry_bytes"] == 4
    strings = [text(rng, rng.randrange(0, 40), b"abcdefghijklmnopqrstuvwxyz0123456789") for _ in range(300)]
    for k in range(0, 300, 7):
        p = pats[k * 31 % 10000]
        at = rng.randrange(0, len(strings[k]) + 1)
        strings[k] = strings[k][:at] + p + strings[k][at:]
    want, far = check_set(core, hs, strings, rng=rng)
    assert len(want) >= 43 and far > 0
    check_set(core, hs, strings, False, "scattered", invert=True, rng=rng)
    hs.free()


def test_all_256_byte_values_as_patterns(core):
    """no byte is left for class 0: 256 classes, not 257"""
    hs = HostSet(core, [bytes([x, x]) for x in range(256)])
    assert hs.info["classes"] == 256 and hs.info["states"] == 258
    strings = [bytes([x, 255 - x, x]) for x in range(256)] + [b"\x00\x00", b"\xff\xff", b"\x7f\x80\x80"]
    check_set(core, hs, strings, want_selected=[256, 257, 258])
    hs.free()
    check(core, [b"ABC", b"abc", b"[", b"{"], [bytes([x]) for x in range(256) if not 65 <= x < 91], nocase=True, want_selected=[0, 1, 2, 3], every=False)


def test_2000_random_cases(core):
    rng = random.Random(2000)
    alphabets = (b"ab", b"abc", b"abAB \xc3\x84\xa4", b"abcdefgh", bytes(range(256)))
    for case in range(2000):
        alphabet = rng.choice(alphabets)
        n = rng.choice((1, 5, 30, 64, 65, 130))
        strings = [text(rng, rng.randrange(0, rng.choice((4, 12, 40))), alphabet) for _ in range(n)]
        pats = []
        for _ in range(rng.randrange(1, 41)):
            src = rng.choice(strings)
            if len(src) >= 1 and rng.random() < 0.5:      # from the data — maybe with a changed byte — or random
                o = rng.randrange(0, len(src)); p = bytearray(src[o:o + rng.randrange(1, 7)])
                if rng.random() < 0.3:
                    p[rng.randrange(len(p))] = rng.choice(alphabet)
                pats.append(bytes(p))
            else:
                pats.append(text(rng, rng.randrange(1, 6), alphabet))
        hs = HostSet(core, pats, nocase=rng.random() < 0.3)
        try:
            check_set(core, hs, strings, rng.random() < 0.5, rng.choice(("packed", "scattered")), invert=rng.random() < 0.25, rng=rng)
        finally:
            hs.free()


def test_the_builders_limits(core):
    L = core
    ok, bad = sx.SX_OK, sx.SX_E_INVALID
    assert sx.SX_SELECT_SET_MAX_PATTERNS == 65536 and sx.SX_SELECT_SET_MAX_PATTERN_BYTES == 255 and sx.SX_SELECT_SET_MAX_TOTAL_BYTES == 1 << 20
    # n_patterns outside 1..65536
    assert create_rc(L, [(b"a", 1)], n=0) == bad
    assert create_rc(L, [(b"a", 1)]) == ok
    many = [(b"ab", 2)] * 65537
    assert create_rc(L, many, n=65536) == ok
    assert create_rc(L, many, n=65537) == bad
    # a length outside 1..255
    long_one = b"q" * 256
    assert create_rc(L, [(long_one, 0)]) == bad
    assert create_rc(L, [(long_one, 1)]) == ok
    assert create_rc(L, [(long_one, 255)]) == ok
    assert create_rc(L, [(long_one, 256)]) == bad
    assert create_rc(L, [(b"ok", 2), (long_one, 256)]) == bad
    # a total above 1 MiB: 4112 x 255 = 1 MiB - 16
    full = [(long_one, 255)] * 4112
    assert create_rc(L, full + [(long_one, 16)]) == ok
    assert create_rc(L, full + [(long_one, 17)]) == bad
    assert create_rc(L, full + [(long_one, 16), (b"a", 1)]) == bad
    # a NULL pointer
    assert create_rc(L, [(None, 3)]) == bad
    assert create_rc(L, [(b"ok", 2), (None, 1)]) == bad
    rc = C.c_int(99)
    assert L.sxs_selset_create(None, 1, 0, C.byref(rc)) is None and rc.value == bad
    # any flag but the fold
    assert create_rc(L, [(b"a", 1)], flags=NOCASE) == ok
    assert create_rc(L, [(b"a", 1)], flags=sx.SX_SELECT_INVERT) == bad
    assert create_rc(L, [(b"a", 1)], flags=4) == bad
    assert create_rc(L, [(b"a", 1)], flags=NOCASE | 1 << 31) == bad
