"""The selection by compiled regular expressions (sx_select_regex_create, sx_result_select_regex_device): the regex compiler
(stringsext_amd/csrc/sx_selre_build.cpp) and the match core (sx_selre_core.hpp) compiled as plain host C++ and driven the way
sx_selre_dev.hip drives them (tests/native/selre_core_host.cpp: the first lds_states rows in a place of their own, wavefront after
wavefront rounds of one step per active lane, the ballot; then the list selection's scan, placement and ordered gather), against
Python's re.search over the strings — every pattern rendered for Python with `$` as `\\Z`, folded sets with re.IGNORECASE.  The
expected value never comes from the code under test.  The source arena ends where a page without access begins: the core may
read nothing behind the last string, not even to decide `$`."""
import ctypes as C
import hashlib
import os
import random
import re
import subprocess

import pytest

import stringsext_amd as sx
from test_select_core import fields, lay_out, records, text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "stringsext_amd", "csrc")
NOCASE = sx.SX_SELECT_ASCII_NOCASE
DEPS = [os.path.join(ROOT, "include", "stringsext_amd.h"), os.path.join(NATIVE, "guarded_host.hpp"), os.path.join(NATIVE, "select_pass2_host.hpp")] + [os.path.join(CSRC, f) for f in (
    "sx_selre_build.cpp", "sx_selre_build.hpp", "sx_selre_front.hpp", "sx_selre_core.hpp", "sx_selset_build.hpp", "sx_select_core.hpp", "sx_result_core.hpp")]


def built(out, src, flags):
    """(as tests/test_select_core.py builds its harness: g++ on one file, rebuilt when a source is newer)"""
    out, src = os.path.join(NATIVE, out), os.path.join(NATIVE, src)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in DEPS + [src]):
        tmp = f"{out}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + ["-o", tmp, src])
        os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def core():
    L = C.CDLL(built("libselre_core_host.so", "selre_core_host.cpp", ["-O2", "-fPIC", "-shared"]))
    u64p = C.POINTER(C.c_uint64)
    L.sxs_selre_create.restype = C.c_void_p
    L.sxs_selre_create.argtypes = [C.POINTER(sx.Pattern), C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.c_char_p, C.c_uint32]
    L.sxs_selre_free.restype, L.sxs_selre_free.argtypes = None, [C.c_void_p]
    L.sxs_selre_info.restype = None
    L.sxs_selre_info.argtypes = [C.c_void_p, C.POINTER(sx.SelectRegexInfo), C.POINTER(C.c_uint32)]
    L.sxs_selre_table.restype, L.sxs_selre_table.argtypes = C.c_uint64, [C.POINTER(sx.Pattern), C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64]
    L.sxs_selre_select_host.restype = C.c_int
    L.sxs_selre_select_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                        C.c_uint64, u64p, u64p, u64p, u64p, u64p]
    L.sxs_guarded.restype, L.sxs_guarded.argtypes = C.c_void_p, [C.c_uint64, C.POINTER(C.c_void_p), u64p]
    L.sxs_unmap.restype, L.sxs_unmap.argtypes = None, [C.c_void_p, C.c_uint64]
    return L


def to_python(p):
    """the pattern as Python reads it: an unescaped `$` outside a class is `\\Z`"""
    out, i, in_class = bytearray(), 0, False
    while i < len(p):
        c = p[i:i + 1]
        if c == b"\\":
            out += p[i:i + 2]; i += 2; continue
        if in_class:
            in_class = c != b"]"
        elif c == b"[":
            in_class = True
        elif c == b"$":
            out += b"\\Z"; i += 1; continue
        out += c; i += 1
    return bytes(out)


def oracle(patterns, nocase):
    res = [re.compile(to_python(p), re.IGNORECASE if nocase else 0) for p in patterns]
    return lambda s: any(r.search(s) is not None for r in res)


def create(L, pats, n=None, flags=0):
    """(handle or None, selre_build's code, its text) for (bytes, len) pairs"""
    arr = (sx.Pattern * max(1, len(pats)))(*[sx.Pattern(p, ln) for p, ln in pats])
    rc, err = C.c_int(99), C.create_string_buffer(512)
    h = L.sxs_selre_create(arr, len(pats) if n is None else n, flags, C.byref(rc), err, 512)
    assert bool(h) == (rc.value == sx.SX_OK)
    return h, rc.value, err.value.decode(errors="replace")


def create_rc(L, pats, n=None, flags=0):
    h, rc, err = create(L, pats, n, flags)
    if h:
        L.sxs_selre_free(h)
    return rc, err


class HostRegex:
    """a set as the builder makes it; .info: sx_select_regex_info's fields plus end_first, stop_first, matched, root_end"""

    def __init__(self, L, patterns, nocase=False):
        self.L, self.patterns, self.nocase = L, [bytes(p) for p in patterns], nocase
        self.h, rc, err = create(L, [(p, len(p)) for p in self.patterns], flags=NOCASE if nocase else 0)
        assert rc == sx.SX_OK and self.h, (rc, err, self.patterns)
        i, shape = sx.SelectRegexInfo(), (C.c_uint32 * 4)()
        L.sxs_selre_info(self.h, C.byref(i), shape)
        self.info = dict({k: getattr(i, k) for k, _ in sx.SelectRegexInfo._fields_},
                         end_first=shape[0], stop_first=shape[1], matched=shape[2], root_end=shape[3])
        # what the header promises of every set
        f = self.info
        assert f["n_patterns"] == len(self.patterns) and f["nocase"] == int(nocase)
        assert 1 <= f["classes"] <= 256 and 1 <= f["states"] <= sx.SX_SELECT_REGEX_MAX_STATES
        assert f["table_bytes"] == f["states"] * f["classes"] * 2
        assert f["lds_states"] == min(f["states"], 48 * 1024 // (f["classes"] * 2)) and f["lds_states"] * f["classes"] * 2 <= 48 * 1024
        assert f["end_first"] <= f["stop_first"] <= f["states"] <= f["stop_first"] + 2
        assert f["end_states"] == f["stop_first"] - f["end_first"] + f["root_end"]

    def free(self):
        self.L.sxs_selre_free(self.h)
        self.h = None


def check_set(L, hr, strings, packed=True, layout="packed", invert=False, rng=None, want_selected=None):
    """hr over `strings` laid out as `layout`, against Python's re; returns (the selected indices, steps outside "LDS", all steps)"""
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
        found = oracle(hr.patterns, hr.nocase)
        want = [i for i, s in enumerate(strings) if found(s) != invert]
        if want_selected is not None:
            assert want == list(want_selected), (hr.patterns, want, list(want_selected))     # (the case is what its author meant)
        total = sum(len(strings[i]) for i in want)
        out = ((sx.Finding16 if packed else sx.Finding) * max(1, n))()
        raw = C.create_string_buffer(b"\xEE" * (total + 64), total + 64)
        waves = (n + 63) // 64
        masks = (C.c_uint64 * (waves + 1))()
        n_sel, sel_bytes, far_steps, steps = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        rc = L.sxs_selre_select_host(hr.h, C.addressof(arr), n, int(packed), base, int(invert), C.addressof(out), C.addressof(raw), total,
                                     masks, C.byref(n_sel), C.byref(sel_bytes), C.byref(far_steps), C.byref(steps))
        assert rc == 0, rc
        got = [w * 64 + b for w in range(waves) for b in range(64) if masks[w] >> b & 1] if n else []
        assert got == want, (hr.patterns, hr.nocase, invert, [(i, strings[i]) for i in sorted(set(got) ^ set(want))[:5]], len(got), len(want))
        assert (n_sel.value, sel_bytes.value) == (len(want), total)
        assert steps.value <= sum(len(s) for s in strings)
        out_arena = raw.raw
        assert out_arena[total:] == b"\xEE" * 64, "bytes behind the selected strings were written"
        off = 0
        for k, i in enumerate(want):
            assert fields(out[k], packed) == fields(arr[i], packed), (k, i)           # every record unchanged except str_off
            assert out[k].str_off == off, (k, out[k].str_off, off)                  # back to back, in record order
            assert out_arena[off:off + len(strings[i])] == strings[i], (k, i)
            off += len(strings[i])
        return want, far_steps.value, steps.value
    finally:
        L.sxs_unmap(region, region_bytes)


def check(L, strings, patterns, nocase=False, want_selected=None, every=True, **kw):
    """one set over both record types and both layouts (every=False: packed records, back to back, only)"""
    if isinstance(patterns, bytes):
        patterns = [patterns]
    hr = HostRegex(L, patterns, nocase)
    try:
        want = None
        for packed in ((True, False) if every else (True,)):
            for layout in (("packed", "scattered") if every else ("packed",)):
                want, _, _ = check_set(L, hr, strings, packed, layout, want_selected=want_selected, **kw)
        return want
    finally:
        hr.free()


# ---- 1. hand-written cases

def test_anchors_at_both_ends_and_in_mid_pattern(core):
    strings = [b"abc", b"xabc", b"abcx", b"ac", b"bc", b"xbc", b"xac", b"a", b"b", b"", b"ab", b"ba", b"c"]
    check(core, strings, b"^abc", want_selected=[0, 2])
    check(core, strings, b"abc$", want_selected=[0, 1])
    check(core, strings, b"^abc$", want_selected=[0])
    check(core, strings, b"(^a|b)c", want_selected=[0, 1, 2, 3, 4, 5])   # "xac": the a is not at the start
    check(core, strings, b"a$|b", want_selected=[0, 1, 2, 4, 5, 7, 8, 10, 11])
    check(core, strings, b"a^b", want_selected=[])
    check(core, strings, b"a$b", want_selected=[])
    check(core, strings, b"(?:^|x)a", want_selected=[0, 1, 2, 3, 6, 7, 10])
    check(core, strings, b"c(?:$|x)", want_selected=[0, 1, 2, 3, 4, 5, 6, 12])
    check(core, strings, b"^^a$$", want_selected=[7])
    check(core, strings, [b"^b", b"c$"], want_selected=[0, 1, 3, 4, 5, 6, 8, 11, 12])
    check(core, [b"$", b"a$", b"^", b"x^y", b"a"], rb"\$$", want_selected=[0, 1])
    check(core, [b"$", b"a$", b"^", b"x^y", b"a"], rb"[$^]", want_selected=[0, 1, 2, 3])
    check(core, [b"$", b"a$", b"^", b"x^y", b"a"], rb"^\^", want_selected=[2])
    # no "in front of a trailing newline" rule: `$` is behind the last byte
    check(core, [b"ab\n", b"ab", b"ab\n\n", b"\nab"], b"ab$", want_selected=[1, 3])
    check(core, [b"ab\n", b"ab", b"\nab", b"x\nab"], b"^ab", want_selected=[0, 1])       # and no line rule for `^` either


def test_the_empty_string_is_decided_by_the_root(core):
    strings = [b"", b"a", b"b", b"", b"aa"]
    check(core, strings, b"a*", want_selected=[0, 1, 2, 3, 4])
    check(core, strings, b"^$", want_selected=[0, 3])
    check(core, strings, b"^", want_selected=[0, 1, 2, 3, 4])
    check(core, strings, b"$", want_selected=[0, 1, 2, 3, 4])
    check(core, strings, b"x", want_selected=[])
    check(core, strings, b"()", want_selected=[0, 1, 2, 3, 4])
    check(core, strings, b"^(|a)$", want_selected=[0, 1, 3])
    check(core, strings, b"^a*$", want_selected=[0, 1, 3, 4])
    check(core, strings, b"^$", invert=True, want_selected=[1, 2, 4])
    check(core, strings, b"$^", want_selected=[0, 3])
    check(core, [b""], b"a|", want_selected=[0])
    check(core, [b""] * 65, b"^$", want_selected=list(range(65)))
    for p, shape in ((b"a*", (1, 0, 0)), (b"^", (1, 0, 0)), (b"a^b", (1, 0, None)), (b"^$", (2, 1, None))):
        hr = HostRegex(core, [p])
        assert hr.info["states"] == shape[0] and hr.info["root_end"] == shape[1], (p, hr.info)
        if shape[2] == 0:
            assert hr.info["matched"] == 0 and hr.info["stop_first"] == 0        # the root is `matched`: no byte is read
        hr.free()


def test_the_dot_matches_every_byte_but_0x0a(core):
    strings = [bytes([x]) for x in range(256)]
    check(core, strings, b".", want_selected=[x for x in range(256) if x != 10])
    check(core, strings, b"^.$", want_selected=[x for x in range(256) if x != 10])
    check(core, strings, b"[.]", want_selected=[46])
    check(core, strings, rb"\.", want_selected=[46])
    check(core, [b"a\nb", b"ab", b"a\n", b"\n", b"a\n\nb", b"axb"], b"a.b", want_selected=[5])
    check(core, [b"a\nb", b"ab", b"a\n", b"\n", b"a\n\nb", b"axb"], b"a.*b", want_selected=[1, 5])


def test_every_shorthand_against_all_256_byte_values(core):
    strings = [bytes([x]) for x in range(256)]
    digit = set(range(48, 58))
    word = digit | set(range(65, 91)) | set(range(97, 123)) | {95}
    space = {32, 9, 10, 11, 12, 13}
    every = set(range(256))
    for letter, members in ((b"d", digit), (b"w", word), (b"s", space)):
        lower, upper = b"\\" + letter, b"\\" + letter.upper()
        for nocase in (False, True):
            check(core, strings, lower, nocase, want_selected=sorted(members), every=False)
            check(core, strings, upper, nocase, want_selected=sorted(every - members), every=False)
            check(core, strings, b"[" + lower + b"]", nocase, want_selected=sorted(members), every=False)
            check(core, strings, b"[^" + lower + b"]", nocase, want_selected=sorted(every - members), every=False)
            check(core, strings, b"[" + upper + b"]", nocase, want_selected=sorted(every - members), every=False)
            check(core, strings, b"[^" + upper + b"]", nocase, want_selected=sorted(members), every=False)
            check(core, strings, b"[" + lower + b"#-]", nocase, want_selected=sorted(members | {35, 45}), every=False)
    check(core, strings, rb"[\d\s]", want_selected=sorted(digit | space), every=False)
    check(core, strings, rb"[^\W\d_]", want_selected=sorted(word - digit - {95}), every=False)
    check(core, strings, rb"[\t\n\r\f\v]", want_selected=[9, 10, 11, 12, 13], every=False)
    check(core, strings, rb"\t|\n|\r|\f|\v", want_selected=[9, 10, 11, 12, 13], every=False)
    check(core, strings, rb"\x00|\xfF|[\x7f-\x81]", want_selected=[0, 127, 128, 129, 255], every=False)
    check(core, strings, rb"\*|\]|\\|\-|\ |\_|\}", want_selected=sorted(b"*]\\- _}"), every=False)
    check(core, strings, rb"[a\-c]|[-x]|[y-]", want_selected=sorted(b"a-cxy"), every=False)
    check(core, strings, rb"[\]\[^]", want_selected=sorted(b"][^"), every=False)
    check(core, strings, rb"[+-\-]", want_selected=[43, 44, 45], every=False)            # a range that ends with '-'
    check(core, strings, rb"}|]", want_selected=sorted(b"}]"), every=False)              # literals outside a class
    check(core, strings, rb"[^\x00-\xff]", want_selected=[], every=False)                 # the empty set
    check(core, strings, b"[^\n]", want_selected=[x for x in range(256) if x != 10], every=False)


def test_counted_repeats_and_their_lazy_forms(core):
    strings = [b"a" * k for k in range(7)] + [b"b" + b"a" * k + b"b" for k in range(7)]
    for lazy in (b"", b"?"):
        check(core, strings, b"^a{3}" + lazy + b"$", want_selected=[3])
        check(core, strings, b"^a{2,}" + lazy + b"$", want_selected=[2, 3, 4, 5, 6])
        check(core, strings, b"^a{2,4}" + lazy + b"$", want_selected=[2, 3, 4])
        check(core, strings, b"^a{,2}" + lazy + b"$", want_selected=[0, 1, 2])
        check(core, strings, b"ba{3}" + lazy + b"b", want_selected=[10])
        check(core, strings, b"ba{2,}" + lazy + b"b", want_selected=[9, 10, 11, 12, 13])
        check(core, strings, b"ba{2,4}" + lazy + b"b", want_selected=[9, 10, 11])
        check(core, strings, b"ba{,2}" + lazy + b"b", want_selected=[7, 8, 9])
        check(core, strings, b"ba*" + lazy + b"b", want_selected=list(range(7, 14)))
        check(core, strings, b"ba+" + lazy + b"b", want_selected=list(range(8, 14)))
        check(core, strings, b"ba?" + lazy + b"b", want_selected=[7, 8])
    check(core, strings, b"^a{0}$", want_selected=[0])
    check(core, strings, b"^(?:a{2}){1,2}$", want_selected=[2, 4])
    check(core, strings, b"^(a|b){9}$", want_selected=[])
    check(core, strings, b"^(ba{5}b|a{6})$", want_selected=[6, 12])
    check(core, strings, b"^(a*)*$", want_selected=list(range(7)))
    check(core, strings, b"^(a|)+$", want_selected=list(range(7)))
    check(core, [b"x" * 254, b"x" * 255, b"x" * 256], b"^x{255}$", want_selected=[1])


def test_utf8_sequences_are_bytes_and_a_quantifier_binds_one_byte(core):
    strings = ["Привет мир".encode(), "привет".encode(), "日本語".encode(), "テスト".encode(), b"\xd0", b"\xd1\x80", "naïve café".encode(),
               b"plain", "é".encode(), b"\xc3\xa9\xa9", b"\xc3", "éé".encode()]
    check(core, strings, "мир".encode(), want_selected=[0])
    check(core, strings, "^привет$".encode(), want_selected=[1])
    check(core, strings, b"\xd0", want_selected=[0, 1, 4])
    check(core, strings, "é$".encode(), want_selected=[6, 8, 11])
    check(core, strings, "^é+$".encode(), want_selected=[8, 9])                    # C3 A9+: the + binds A9 alone
    check(core, strings, "^(é)+$".encode(), want_selected=[8, 11])
    check(core, strings, "^é?$".encode(), want_selected=[8, 10])                   # C3 (A9)?
    check(core, strings, b"[\xa9-\xbf]$", want_selected=[6, 8, 9, 11])
    check(core, strings, rb"^[^\x00-\x7f]+$", want_selected=[1, 2, 3, 4, 5, 8, 9, 10, 11])
    check(core, strings, b"\\\xc3\\\xa9", want_selected=[6, 8, 9, 11])             # a backslash in front of a byte >= 0x80: that byte
    check(core, strings, "^...$".encode(), want_selected=[9])               # `.` is a byte: three of them


def test_the_fold_is_re_ignorecase_on_a_bytes_pattern(core):
    strings = [b"z", b"A", b"a", b"Z", b"[", b"`", b"_", b"m", b"M", b"\xc3\x84", b"\xc3\xa4", b"{", b"@", b"0"]
    check(core, strings, b"^[Z-a]$", want_selected=[2, 3, 4, 5, 6])
    check(core, strings, b"^[Z-a]$", nocase=True, want_selected=[0, 1, 2, 3, 4, 5, 6])
    check(core, strings, b"^[^Z-a]$", want_selected=[0, 1, 7, 8, 11, 12, 13])
    check(core, strings, b"^[^Z-a]$", nocase=True, want_selected=[7, 8, 11, 12, 13])
    check(core, strings, b"^m$", nocase=True, want_selected=[7, 8])
    check(core, strings, b"^M$", nocase=True, want_selected=[7, 8])
    check(core, strings, b"^M$", want_selected=[8])
    check(core, strings, b"[^m]", nocase=True, want_selected=[0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13])
    check(core, strings, b"^\xc3\x84$", nocase=True, want_selected=[9])             # no byte >= 0x80 is folded
    check(core, strings, rb"^[\xa0-\xff][\x80-\x9f]$", nocase=True, want_selected=[9])
    check(core, strings, rb"^\x4d$", nocase=True, want_selected=[7, 8])
    check(core, strings, b"^[@-Z]$", nocase=True, want_selected=[0, 1, 2, 3, 7, 8, 12])
    check(core, strings, b"^[`-z]$", nocase=True, want_selected=[0, 1, 2, 3, 5, 7, 8])
    check(core, [b"MiXeD CaSe", b"mixed case", b"MIXED CASE", b"mixed_case"], b"^mIxEd CASE$", nocase=True, want_selected=[0, 1, 2])
    a, b = HostRegex(core, [b"Ab"], nocase=True), HostRegex(core, [b"aB|AB|ab"], nocase=True)
    assert (a.info["states"], a.info["classes"]) == (b.info["states"], b.info["classes"]) == (3, 3)
    a.free(); b.free()


# ---- 2. the edges of a record and of a wavefront

@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_record_counts_around_a_wavefront(core, n, packed):
    rng = random.Random(70 + n)
    strings = [text(rng, rng.randrange(0, 24), b"abc") for _ in range(n)]
    strings[-1] = b"the last one"
    if n >= 65:
        strings[62:65] = [b"..ab", b"....ab", b"cd...."]      # records 63 and 64: a wavefront's last and the next one's first
    some, none, every = HostRegex(core, [b"ab+c|^c", b"one$"]), HostRegex(core, [b"#"]), HostRegex(core, [b"x*"])
    for layout in ("packed", "scattered"):
        for invert in (False, True):
            check_set(core, some, strings, packed, layout, invert=invert, rng=rng)
        a, _, _ = check_set(core, some, strings, packed, layout, rng=rng)
        b, _, _ = check_set(core, some, strings, packed, layout, invert=True, rng=rng)
        assert sorted(a + b) == list(range(n)) and n - 1 in a                       # invert partitions the records
        check_set(core, none, strings, packed, layout, rng=rng, want_selected=[])                          # nothing selected
        check_set(core, none, strings, packed, layout, invert=True, rng=rng, want_selected=list(range(n)))
        check_set(core, every, strings, packed, layout, rng=rng, want_selected=list(range(n)))              # everything selected
        check_set(core, every, strings, packed, layout, invert=True, rng=rng, want_selected=[])
    for hr in (some, none, every):
        hr.free()
    if n >= 65:
        assert b"abcd" in b"".join(strings[63:65])
        base = [i for i, s in enumerate(strings) if b"abcd" in s]
        check(core, strings, b"abcd", want_selected=base)                            # only across the two strings: selected nowhere
        assert 63 not in base and 64 not in base
        want = check(core, strings, b"ab$")                                          # ....ab is followed by c, not by the end of the arena
        assert 62 in want and 63 in want
        want = check(core, strings, b"ab$|abx")
        assert 63 in want
        want = check(core, strings, b"^cd")
        assert 64 in want and 63 not in want
        assert check(core, strings, b"^b$") == [i for i, s in enumerate(strings) if s == b"b"]


def test_a_match_never_spans_two_records_and_a_dollar_never_looks_ahead(core):
    strings = [b"....ab", b"x", b"cd....", b"a", b"b", b"", b"abc", b"", b"d", b"ab"]
    check(core, strings, b"abx", want_selected=[])
    check(core, strings, b"ab$", want_selected=[0, 9])          # the last string ends where the inaccessible page begins
    check(core, strings, b"^cd", want_selected=[2])
    check(core, strings, b"xcd", want_selected=[])
    check(core, strings, b"^d$", want_selected=[8])
    check(core, strings, b"b.*d", want_selected=[])
    check(core, strings, b"^$", want_selected=[5, 7])
    rng = random.Random(9)
    strings = [text(rng, rng.randrange(4, 20), b"abcdefghijklmnopqrstuvwxyz") for _ in range(150)]
    spans = [strings[i][-3:] + strings[i + 1][:3] for i in range(149)]
    spans = [p for p in spans if not any(p in s for s in strings)][:64]
    assert len(spans) == 64
    check(core, strings, spans, want_selected=[], every=False)
    check(core, strings, [p[:3] + b".?" + p[3:] for p in spans], want_selected=[], every=False)
    tails = [p[:3] + b"$" for p in spans]
    want = check(core, strings, tails, every=False)
    assert want == [i for i, s in enumerate(strings) if any(s.endswith(p[:3]) for p in spans)] and len(want) >= 64


def test_a_lane_stops_at_dead_and_at_matched(core):
    strings = [b"x" + b"a" * 500, b"abc" + b"y" * 500, b"ab" + b"y" * 500]
    hr = HostRegex(core, [b"^abc"])
    want, _, steps = check_set(core, hr, strings, want_selected=[1])
    assert steps == 1 + 3 + 3                                    # a mismatch, the match, the mismatch at the third byte
    assert hr.info["states"] == 5 and hr.info["stop_first"] == 3 and hr.info["matched"] == 4 and hr.info["end_states"] == 0
    hr.free()
    hr = HostRegex(core, [b"^abc$"])
    want, _, steps = check_set(core, hr, strings, want_selected=[])
    assert steps == 1 + 4 + 3 and hr.info["matched"] == 0xFFFFFFFF and hr.info["end_states"] == 1
    hr.free()


def test_rows_in_lds_and_rows_in_the_table(core):
    rng = random.Random(4800)
    words = [text(rng, 12, b"abcdefghijklmnopqrstuvwxyz") for _ in range(400)]
    pats = [b"|".join(words[k:k + 40]) for k in range(0, 400, 40)]
    hr = HostRegex(core, pats)
    assert hr.info["states"] > hr.info["lds_states"] > 0 and hr.info["classes"] == 27, hr.info      # 26 letters and every other byte
    strings = [text(rng, rng.randrange(0, 60), b"abcdefghijklmnopqrstuvwxyz") for _ in range(600)]
    for k in range(0, 600, 3):
        at = rng.randrange(0, len(strings[k]) + 1)
        strings[k] = strings[k][:at] + words[k * 7 % 400][:rng.choice((12, 12, 11, 8))] + strings[k][at:]
    for packed, layout in ((True, "packed"), (False, "scattered")):
        want, far, _ = check_set(core, hr, strings, packed, layout, rng=rng)
        assert 50 < len(want) < len(strings) and far > 0
        check_set(core, hr, strings, packed, layout, invert=True, rng=rng)
    hr.free()


# ---- 3. random cases

SPECIAL = b".^$*+?{}[]\\|()"


def is_alnum(x):
    return 48 <= x < 58 or 65 <= x < 91 or 97 <= x < 123


def render_byte(rng, x, in_class=False):
    if is_alnum(x):
        return bytes([x])
    how = rng.randrange(3)
    if how == 0 or x == 10 and how == 2:
        return b"\\x%02x" % x
    if how == 1 or in_class or x in SPECIAL or x in b"-":
        return b"\\" + bytes([x])
    return bytes([x])


class Tree:
    """a random syntax tree: render() for the library (Python reads the same text, `$` apart), sample() a string it matches"""

    def __init__(self, rng, alphabet, depth):
        self.rng, self.alphabet = rng, alphabet
        self.node = self.make(depth)

    def make(self, depth):
        rng = self.rng
        kind = rng.choice(("lit", "lit", "lit", "class", "dot", "short", "anchor", "empty") if depth == 0 else
                          ("cat", "cat", "alt", "rep", "rep", "lit", "class", "group"))
        if kind == "lit":
            return ("lit", rng.choice(self.alphabet))
        if kind == "class":
            items = []
            for _ in range(rng.randrange(1, 4)):
                a, b = sorted((rng.choice(self.alphabet), rng.choice(self.alphabet)))
                r = rng.random()
                items.append(("range", a, b) if r < 0.3 else ("short", rng.choice(b"dDwWsS")) if r < 0.4 else ("lit", a))
            return ("class", rng.random() < 0.3, items)
        if kind == "short":
            return ("short", rng.choice(b"dDwWsS"))
        if kind == "anchor":
            return ("anchor", rng.choice(b"^$"))
        if kind in ("dot", "empty"):
            return (kind,)
        if kind in ("cat", "alt"):
            return (kind, [self.make(depth - 1) for _ in range(rng.randrange(2, 4))])
        if kind == "group":
            return ("group", rng.random() < 0.5, self.make(depth - 1))
        lo, hi = sorted((rng.randrange(0, 4), rng.randrange(0, 4)))
        form = rng.choice(("*", "+", "?", "{m}", "{m,}", "{m,n}", "{,n}"))
        return ("rep", form, lo, hi, rng.random() < 0.2, self.make(depth - 1))

    def render(self, node=None):
        node, rng = node or self.node, self.rng
        kind = node[0]
        if kind == "lit":
            return render_byte(rng, node[1])
        if kind == "class":
            out = b"[^" if node[1] else b"["
            for item in node[2]:
                if item[0] == "range":
                    out += render_byte(rng, item[1], True) + b"-" + render_byte(rng, item[2], True)
                elif item[0] == "short":
                    out += b"\\" + bytes([item[1]])
                else:
                    out += render_byte(rng, item[1], True)
            return out + b"]"
        if kind == "short":
            return b"\\" + bytes([node[1]])
        if kind == "anchor":
            return bytes([node[1]])
        if kind == "dot":
            return b"."
        if kind == "empty":
            return b"()"
        if kind == "cat":
            return b"".join(self.render(k) if k[0] != "alt" else b"(?:" + self.render(k) + b")" for k in node[1])
        if kind == "alt":
            return b"|".join(self.render(k) for k in node[1])
        if kind == "group":
            return (b"(" if node[1] else b"(?:") + self.render(node[2]) + b")"
        _, form, lo, hi, lazy, kid = node
        q = {"*": b"*", "+": b"+", "?": b"?", "{m}": b"{%d}" % lo, "{m,}": b"{%d,}" % lo, "{m,n}": b"{%d,%d}" % (lo, hi), "{,n}": b"{,%d}" % hi}[form]
        return b"(?:" + self.render(kid) + b")" + q + (b"?" if lazy else b"")

    def sample(self, node=None):
        node, rng = node or self.node, self.rng
        kind = node[0]
        if kind == "lit":
            return bytes([node[1]])
        if kind in ("class", "short", "dot"):
            return bytes([rng.choice(self.alphabet)])        # (a guess: it need not fit)
        if kind in ("anchor", "empty"):
            return b""
        if kind == "cat":
            return b"".join(self.sample(k) for k in node[1])
        if kind == "alt":
            return self.sample(rng.choice(node[1]))
        if kind == "group":
            return self.sample(node[2])
        _, form, lo, hi, _, kid = node
        lo, hi = {"*": (0, 2), "+": (1, 3), "?": (0, 1), "{m}": (lo, lo), "{m,}": (lo, lo + 2), "{m,n}": (lo, hi), "{,n}": (0, hi)}[form]
        return b"".join(self.sample(kid) for _ in range(rng.randrange(lo, hi + 1)))


ALPHABETS = (b"ab", b"abc", b"abAB_ 9\n", bytes(range(256)))


def random_case(rng):
    """(patterns, nocase, invert, strings)"""
    alphabet = rng.choice(ALPHABETS)
    trees = [Tree(rng, alphabet, rng.randrange(0, 5)) for _ in range(rng.choice((1, 1, 1, 2, 3)))]
    pats = [t.render() for t in trees]
    assert all(1 <= len(p) <= 1024 for p in pats)
    strings = []
    for _ in range(rng.choice((1, 5, 20, 64, 65, 70))):
        r = rng.random()
        if r < 0.5:
            s = text(rng, rng.randrange(0, rng.choice((4, 12, 41))), alphabet)
        else:
            s = rng.choice(trees).sample()
            if r < 0.7:
                s = text(rng, rng.randrange(0, 4), alphabet) + s + text(rng, rng.randrange(0, 4), alphabet)
            elif r < 0.8 and s:
                a, b = sorted((rng.randrange(len(s) + 1), rng.randrange(len(s) + 1)))
                s = s[a:b]
        strings.append(s[:40])
    return pats, rng.random() < 0.3, rng.random() < 0.25, strings


def test_2400_random_cases(core):
    rng = random.Random(2400)
    hits = misses = 0
    for case in range(2400):
        pats, nocase, invert, strings = random_case(rng)
        hr = HostRegex(core, pats, nocase)         # (a refused case fails here: the generator stays inside the language and the limits)
        try:
            want, _, _ = check_set(core, hr, strings, rng.random() < 0.5, rng.choice(("packed", "scattered")), invert=invert, rng=rng)
            hits += len(want) if not invert else len(strings) - len(want)
            misses += len(strings) - len(want) if not invert else len(want)
        finally:
            hr.free()
    assert hits > 5000 and misses > 5000, (hits, misses)     # the cases decide something


# ---- 4. minimisation

def shape(core, p, nocase=False):
    hr = HostRegex(core, [p] if isinstance(p, bytes) else p, nocase)
    f = hr.info
    hr.free()
    return f["states"], f["classes"]


def test_equivalent_patterns_give_the_same_automaton(core):
    for group in ((b"[ab]*abb$", b"(a|b)*abb$", b"(?:b|a)*abb$", b"abb$"),
                  (b"a+", b"aa*", b"a{1,}", b"a", b"a+?", b"(a|aa)"),
                  (b"x{2,3}", b"xxx?", b"xx", b"xx|xxx"),
                  (b"colou?r", b"color|colour", b"colo(?:u|)r", [b"color", b"colour"]),
                  (b"^a[\\x00-\\xff]*$", b"^a", b"^a(.|\\n)*$"),
                  (b"a[\\x00-\\xff]*$", b"a")):
        shapes = [shape(core, p) for p in group]
        assert len(set(shapes)) == 1, (group, shapes)
    assert shape(core, b"[ab]*abb$") == (4, 3)        # the textbook DFA of (a|b)*abb: every other byte leads back to the root
    assert shape(core, b"colou?r") == (7, 6)
    for k in (1, 2, 5, 26):
        assert shape(core, bytes(range(97, 97 + k))) == (k + 1, k + 1)      # a literal of k distinct bytes: what selset_build gives it
    for p, ends in ((b"abb", 0), (b"a|b+c", 0), (b"abb$", 1), (b"^$", 1), (b"a$|b$", 1), (b"ab?$", 2), (b"^a*$", 1)):
        hr = HostRegex(core, [p])
        assert hr.info["end_states"] == ends, (p, hr.info)
        hr.free()
    hr = HostRegex(core, [b"^abc"])
    assert hr.info["states"] == 5 and hr.info["stop_first"] == 3          # root, a, ab, dead, matched
    hr.free()


# sha256 of sxs_selre_table's bytes — ten words of SelreTable, the class map, the entries.  The first nine as the harness of the
# commit before the front end moved into sx_selre_front.hpp gave them, the others as commit 046f17a gave them, the last one in
# which each builder had a subset construction, a numbering and a row writer of its own: selre_build's output has not changed by a
# bit.  tests/test_extract_core.py and tests/test_label_core.py pin their builders' tables of the same lists (PINNED_SETS).  Behind
# the nine, one list per branch of a numbering that they leave out: a root that is `dead` and the only state; a root that accepts
# at the end; two starts that differ; 64 patterns; a root with a `here` of its own; 512 pairs of masks (pattern k matches where
# the k-th byte back is an a); a `dead` that is not the root next to states with here != 0; an anchored walk that never dies.
SELRE_PINNED = [
    ([b"abc"], 0, "e6b65c91f276f8dd92a28192f6bcee2737989f8e7c1784f5fc80fdd1b549d95c"),
    ([b"^abc$"], 0, "b3833de49b6d8f4bc8dda30e36da698b346ca39b1c5c39cd9891ea0ad5474c19"),
    ([b"a*"], 0, "e4b60262073c764435e3ca95d0b86ae886493b46949c78fa49456b821f751159"),
    ([b"colou?r", b"gr[ae]y$"], NOCASE, "10cca68cd7cfb89b56be4d5e8b52d7a412acd023100da874d5e7e772ba40a908"),
    ([rb"https?://[^\s/]+(/\S*)?", rb"[\w.+-]+@[\w-]+(\.[\w-]+)+", rb"(\d{1,3}\.){3}\d{1,3}"], 0, "a9ae5668225d5a13ddcbeb54f9619b5d9646b728458580c2b1290d6aa5d8925b"),
    ([b"^[ab]*a[ab]{9}$"], 0, "9db6c4a75880c20e8beb93715326353c7277a02bb9313168f9b44b7396d05caf"),
    ([b"(^a|b)c", b"a$|b", b"x{2,5}y?"], 0, "b9927323b63b40889c1d7fff977a37092ee93e46f8a865cc04bb8b6002211671"),
    ([b"|".join(b"w%03d" % k for k in range(0, 300, 7)), rb"[^\x00-\x7f]{2,4}"], NOCASE, "ee8ec0484ca25f32d857e6fb948d28dd63b422054020b1ff4c869ac99e0b20fa"),
    ([b"(?:a{2,}){2,}b|^$"], 0, "1be0b569cddd33d9c6e6fca74462441f3a0b20b14ebca7bc12c5b9e15439a6f8"),
    ([b"a^b"], 0, "8bf16db43512c567f2ab7c6eb02b5cffb82423018a0dd21107b33ef9adae7fda"),
    ([b"^$"], 0, "7c97c89da018550ff9cab6f036ed78f596e12d23316cdf73fba9cabf3080893a"),
    ([b"^a|b"], 0, "22ef564b907025770706e9b8265998b89bc130688aa1744f6a3d93e86e89e84d"),
    ([b"k%02d;" % p for p in range(63)] + [b"^z+$"], 0, "1c7eb42390e81f581ab9749a953d0dcd2aa0a9021254fcde9de9f84f2deb56f4"),
    ([b"a*", b"b"], 0, "608e1f26fc68c92b7f4d3cfe758eb489aad28d3c9ee68b408260f25627ee6a60"),
    ([b"a[ab]{%d}" % k for k in range(1, 10)], 0, "b8d94a8a57217c119757ec7cb537b918679c378615daf5ea85f7be4518d888d0"),
    ([b"^abc", b"^abd$"], 0, "a0befb8e89d9ee6052911c2f0e5af156f16ccdce02113e015048e3e53203db3a"),
    ([rb"[\x00-\xff]+"], 0, "266667dbafae5b1a1b5291a75b3a9ad5f5d3c8117b57d05d75b5604d7e8a9d85"),
]
PINNED_SETS = [(pats, flags) for pats, flags, _ in SELRE_PINNED]


def test_the_regex_sets_tables_are_unchanged(core):
    shapes = set()
    for pats, flags, digest in SELRE_PINNED:
        arr = (sx.Pattern * len(pats))(*[sx.Pattern(p, len(p)) for p in pats])
        buf = C.create_string_buffer(1 << 22)
        n = core.sxs_selre_table(arr, len(pats), flags, buf, len(buf))
        assert n
        assert hashlib.sha256(buf.raw[:n]).hexdigest() == digest, pats
        states, end_first, stop_first, matched, root_end = (int.from_bytes(buf.raw[4 * k:4 * k + 4], "little") for k in (1, 5, 6, 7, 8))
        shapes.add((states == 1, matched == 0xFFFFFFFF, stop_first + (matched != 0xFFFFFFFF) < states, bool(root_end), end_first < stop_first))
    # every branch of the numbering is among them: the only state `matched` or `dead`, with and without `matched`, `dead`, root_end,
    # end-accepting states
    assert {(True, False), (True, True)} <= {s[:2] for s in shapes} and all({True, False} <= {s[k] for s in shapes if not s[0]} for k in (1, 2, 3, 4)), shapes


# ---- 5. limits and refusals

REFUSED = [  # (pattern, the offset the text names)
    (b"[]a]", 1), (b"[^]a]", 2), (b"[a[b]", 2), (b"[[:alpha:]]", 1), (b"[abc", 0), (b"[a-", 0), (b"[z-a]", 1), (b"[a-\\d]", 3), (b"[\\d-z]", 1),
    (b"[\\b]", 1), (b"[a-[]", 3),
    (b"(?i)a", 0), (b"(?=a)", 0), (b"(?!a)", 0), (b"(?P<n>a)", 0), (b"(?#c)", 0), (b"(?", 0), (b"(a", 0), (b"(?:a", 0), (b"a)", 1), (b"a(b))", 4),
    (b"a**", 2), (b"a*+", 2), (b"a+*", 2), (b"a?+", 2), (b"a*??", 3), (b"a{2}{3}", 4), (b"a{2}*", 4), (b"a+{2}", 2),
    (b"*a", 0), (b"+", 0), (b"?a", 0), (b"a|*b", 2), (b"(*a)", 1), (b"(?:+a)", 3), (b"^*", 1), (b"$+", 1), (b"^{2}", 1), (b"a|$?", 3),
    (b"a{", 1), (b"a{x}", 1), (b"a{1,2", 1), (b"a{,}", 1), (b"a{}", 1), (b"{1}", 0), (b"a{1 }", 1), (b"a{1,2,3}", 1), (b"a{-1}", 1), (b"a|{2}", 2),
    (b"\\b", 0), (b"a\\B", 1), (b"\\A", 0), (b"a\\Z", 1), (b"\\1", 0), (b"\\e", 0), (b"\\z", 0), (b"\\0", 0), (b"\\a", 0), (b"\\N", 0), (b"\\u0041", 0),
    (b"\\x4", 0), (b"\\xg0", 0), (b"ab\\x", 2), (b"a\\", 1), (b"[a\\", 2),
    (b"a{256}", 1), (b"a{3,2}", 1), (b"a{1,256}", 1), (b"a{256,}", 1), (b"a{99999999999}", 1),
]


def test_every_refused_form_names_the_pattern_and_the_offset(core):
    bad = sx.SX_E_INVALID
    for p, off in REFUSED:
        rc, err = create_rc(core, [(p, len(p))])
        assert rc == bad and "pattern 0, offset %d:" % off in err, (p, rc, err)
        rc, err = create_rc(core, [(b"ok", 2), (b"a|b", 3), (p, len(p))], flags=NOCASE)
        assert rc == bad and "pattern 2, offset %d:" % off in err, (p, rc, err)
    for p in (b"a{255}", b"a{0,255}", b"a{3,3}", b"}", b"]", b"a|", b"|", b"()", b"(|)", b"\\{1\\}", b"[{]", b"a{,3}", b"-", b"[a-]", b"\\-", b"(?:)"):
        rc, err = create_rc(core, [(p, len(p))])
        assert rc == sx.SX_OK, (p, err)
        re.compile(to_python(p))


def test_the_builders_limits(core):
    L, ok, bad = core, sx.SX_OK, sx.SX_E_INVALID
    assert (sx.SX_SELECT_REGEX_MAX_PATTERNS, sx.SX_SELECT_REGEX_MAX_PATTERN_BYTES, sx.SX_SELECT_REGEX_MAX_REPEAT) == (64, 1024, 255)
    assert (sx.SX_SELECT_REGEX_MAX_POSITIONS, sx.SX_SELECT_REGEX_MAX_STATES) == (65536, 65536)
    # states
    hr = HostRegex(L, [b"^[ab]*a[ab]{14}$"])
    assert 2 ** 15 <= hr.info["states"] <= 2 ** 15 + 2 and hr.info["classes"] == 3
    strings = [b"a" + b"b" * 14, b"ba" + b"a" * 14, b"b" * 15, b"a" * 14, b"xa" + b"b" * 14, b"a" + b"b" * 13 + b"x", b"abab" * 10, b"ab" * 9 + b"b" * 13]
    check_set(L, hr, strings, want_selected=[0, 1, 7])
    hr.free()
    rc, err = create_rc(L, [(b"^[ab]*a[ab]{16}$", 16)])
    assert rc == bad and "SX_SELECT_REGEX_MAX_STATES" in err, err            # its minimal DFA has 2^17
    # positions
    p = b"((a{255}){255}){255}"
    rc, err = create_rc(L, [(p, len(p))])
    assert rc == bad and "SX_SELECT_REGEX_MAX_POSITIONS" in err, err
    p = b"(((){255}){255}){255}"                                                # nothing but empty groups: refused as well, at once
    rc, err = create_rc(L, [(p, len(p))])
    assert rc == bad and "SX_SELECT_REGEX_MAX_POSITIONS" in err, err
    p = b"^(a{255}){200}"
    assert create_rc(L, [(p, len(p))])[0] == ok                                  # 51 000 positions
    rc, err = create_rc(L, [(p, len(p))] * 2)                                    # all patterns together
    assert rc == bad and "pattern 1" in err and "SX_SELECT_REGEX_MAX_POSITIONS" in err, err
    # n_patterns outside 1..64
    many = [(b"ab", 2)] * 65
    assert create_rc(L, many, n=0)[0] == bad
    assert create_rc(L, many, n=64)[0] == ok
    rc, err = create_rc(L, many, n=65)
    assert rc == bad and "n_patterns" in err
    # a length outside 1..1024
    long_one = b"q" * 1025
    assert create_rc(L, [(long_one, 0)])[0] == bad
    assert create_rc(L, [(long_one, 1)])[0] == ok
    assert create_rc(L, [(long_one, 1024)])[0] == ok
    rc, err = create_rc(L, [(b"ok", 2), (long_one, 1025)])
    assert rc == bad and "pattern 1" in err
    # the repeat
    assert create_rc(L, [(b"a{255}", 6)])[0] == ok
    rc, err = create_rc(L, [(b"a{256}", 6)])
    assert rc == bad and "SX_SELECT_REGEX_MAX_REPEAT" in err
    rc, err = create_rc(L, [(b"a{3,2}", 6)])
    assert rc == bad and "m > n" in err
    # a NULL pointer
    assert create_rc(L, [(None, 3)])[0] == bad
    assert create_rc(L, [(b"ok", 2), (None, 1)])[0] == bad
    rc, err = C.c_int(99), C.create_string_buffer(64)
    assert L.sxs_selre_create(None, 1, 0, C.byref(rc), err, 64) is None and rc.value == bad
    # any flag but the fold
    assert create_rc(L, [(b"a", 1)], flags=NOCASE)[0] == ok
    assert create_rc(L, [(b"a", 1)], flags=sx.SX_SELECT_INVERT)[0] == bad
    assert create_rc(L, [(b"a", 1)], flags=4)[0] == bad
    assert create_rc(L, [(b"a", 1)], flags=NOCASE | 1 << 31)[0] == bad


def nested(inner, quantifier, depth):
    return b"(?:" * depth + inner + (quantifier + b")") * depth


DEEP = [(nested(b"a", b"+", 100), True), (nested(b"a", b"+?", 100), True), (nested(b"a", b"*", 100), True), (nested(b"a", b"{1,}", 100), True),
        (nested(b"ab", b"+", 200), True), (nested(b"a", b"{2,}", 100), False), (nested(b"a", b"{2,3}", 100), False), (nested(b"a", b"{2}", 100), False),
        (b"(" * 200 + b"a" + b")" * 200, True)]


def test_deeply_nested_repeats_compile_at_once_or_are_refused_at_once(core):
    """x+ is ONE copy of x and a branch, so ((a+)+)+... has as many NFA nodes as its count of positions says — 100 levels compile
    to the automaton of `a` —, and (...(a{2,}){2,}...) doubles per level and is refused for positions before anything is built"""
    import time
    for p, compiles in DEEP:
        t0 = time.perf_counter()
        h, rc, err = create(core, [(p, len(p))])
        took = time.perf_counter() - t0
        assert took < 1.0, (p[:20], took)           # (seconds: an NFA that doubled per level would not get here, nor fit the memory)
        if compiles:
            assert rc == sx.SX_OK, (p[:20], err)
            core.sxs_selre_free(h)
        else:
            assert rc == sx.SX_E_INVALID and "pattern 0" in err and "SX_SELECT_REGEX_MAX_POSITIONS" in err, (p[:20], err)
    assert shape(core, nested(b"a", b"+", 100)) == shape(core, nested(b"a", b"{1,}", 100)) == shape(core, b"a") == (2, 2)
    assert shape(core, nested(b"a", b"*", 100)) == (1, 1)
    assert shape(core, nested(b"ab", b"+", 200)) == shape(core, b"ab")
    assert shape(core, b"^" + nested(b"a", b"+", 100) + b"$") == shape(core, b"^a+$")
    strings = [b"", b"a", b"b", b"aaa", b"ba", b"xaby", b"abab", b"ba"]
    check(core, strings, nested(b"a", b"+", 100), want_selected=[1, 3, 4, 5, 6, 7], every=False)
    check(core, strings, b"^" + nested(b"ab", b"+", 50) + b"$", want_selected=[6], every=False)
    # x{m,} is m copies, the last of which loops
    strings = [b"a" * k for k in range(8)]
    check(core, strings, b"^(?:(?:a{2,}){2,})$", want_selected=[4, 5, 6, 7], every=False)
    check(core, strings, b"^(?:aa|aaa){2,}$", want_selected=[4, 5, 6, 7], every=False)
    check(core, strings, b"^(?:a{3,}b?){1,}$", want_selected=[3, 4, 5, 6, 7], every=False)
    assert shape(core, b"a{3,}") == shape(core, b"aaa+") == shape(core, b"aaaa*") == shape(core, b"aaa")


# ---- 6. the builder and the core under the address and undefined-behaviour sanitizers, as a program of their own

def test_a_sanitizer_build_refuses_and_selects_the_same(tmp_path):
    exe = built("selre_build_main", "selre_build_main.cpp", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    rng = random.Random(300)
    cases = []      # (patterns, flags, invert, strings, want: a code or the selected indices)
    for p, _ in REFUSED:
        cases.append(([p], 0, 0, [b"a"], sx.SX_E_INVALID))
    for pats in ([b"ab"] * 65, [b"q" * 1025], [b"a{256}"], [b"a{3,2}"], [b"^[ab]*a[ab]{16}$"], [b"((a{255}){255}){255}"], [b""]):
        cases.append((pats, 0, 0, [b"a"], sx.SX_E_INVALID))
    cases.append(([b"a"], 4, 0, [b"a"], sx.SX_E_INVALID))
    for p, compiles in DEEP:
        strings = [b"", b"a", b"b", b"aaa", b"ba", b"xaby", b"abab"]
        found = oracle([p], False) if compiles else None
        cases.append(([p], 0, 0, strings, [i for i, x in enumerate(strings) if found(x)] if compiles else sx.SX_E_INVALID))
    for _ in range(300):
        pats, nocase, invert, strings = random_case(rng)
        found = oracle(pats, nocase)
        cases.append((pats, NOCASE if nocase else 0, int(invert), strings, [i for i, s in enumerate(strings) if found(s) != invert]))
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for pats, flags, invert, strings, _ in cases:
            f.write("case %d %d\n" % (flags, invert))
            f.writelines("p %s\n" % p.hex() for p in pats)
            f.writelines("s %s\n" % s.hex() for s in strings)
            f.write("end\n")
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-3000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases)
    for line, (pats, flags, invert, strings, want) in zip(lines, cases):
        if isinstance(want, int):
            assert line.startswith("rc %d " % want), (pats, line)
        else:
            assert line.split() == ["sel"] + [str(i) for i in want], (pats, flags, invert, line, want)
