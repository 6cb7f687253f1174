"""The labels of a device-resident result (sx_label_set_create, sx_result_label_device, sx_result_select_labels_device): the label
compiler (stringsext_amd/csrc/sx_label_build.cpp) and the lane functions (sx_label_core.hpp) compiled as plain host C++ and driven
the way sx_label_dev.hip drives them (tests/native/label_core_host.cpp: the first lds_states rows in a place of their own, a grid of
workgroups that strides over the segment, rounds of one step per active lane, the OR over the wavefront, the ballots into the
workgroup's counters and their flush; then label_pick_lane and the list selection's scan, placement and ordered gather), against
Python's re.search PER PATTERN over the strings — every pattern rendered for Python with `$` as `\\Z`, folded sets with
re.IGNORECASE.  No expected value comes from the code under test.  The source arena ends where a page without access begins: the
core may read nothing behind the last string, not even to decide `$`."""
import ctypes as C
import hashlib
import os
import random
import re
import subprocess

import pytest

import stringsext_amd as sx
import test_selre_core as tsc
from test_select_core import fields, lay_out, records, text
from test_selre_core import DEEP, PINNED_SETS, REFUSED, Tree, to_python

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "stringsext_amd", "csrc")
NOCASE = sx.SX_SELECT_ASCII_NOCASE
NEVER = sx.SX_LABEL_NEVER
NONE = 0xFFFFFFFF          # kLabelNone: `dead` where no state is
DEPS = [os.path.join(ROOT, "include", "stringsext_amd.h"), os.path.join(NATIVE, "guarded_host.hpp"), os.path.join(NATIVE, "select_pass2_host.hpp")] + [os.path.join(CSRC, f) for f in (
    "sx_label_build.cpp", "sx_label_build.hpp", "sx_label_core.hpp", "sx_selre_front.hpp", "sx_selset_build.hpp", "sx_select_core.hpp",
    "sx_seltally_core.hpp", "sx_result_core.hpp")]


def built(out, src, flags):
    """(as tests/test_selre_core.py builds its harness: g++ on one file, rebuilt when a source is newer)"""
    out, src = os.path.join(NATIVE, out), os.path.join(NATIVE, src)
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in DEPS + [src]):
        tmp = f"{out}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + ["-o", tmp, src])
        os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def core():
    L = C.CDLL(built("liblabel_core_host.so", "label_core_host.cpp", ["-O2", "-fPIC", "-shared"]))
    u64p = C.POINTER(C.c_uint64)
    L.sxs_label_create.restype = C.c_void_p
    L.sxs_label_create.argtypes = [C.POINTER(sx.Pattern), C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.c_char_p, C.c_uint32]
    L.sxs_label_free.restype, L.sxs_label_free.argtypes = None, [C.c_void_p]
    L.sxs_label_info.restype, L.sxs_label_info.argtypes = None, [C.c_void_p, C.POINTER(sx.LabelSetInfo), u64p]
    L.sxs_label_table.restype, L.sxs_label_table.argtypes = C.c_uint64, [C.c_void_p, C.c_void_p, C.c_uint64]
    L.sxs_label_host.restype = C.c_int
    L.sxs_label_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, u64p, u64p, u64p, u64p, u64p]
    L.sxs_label_pick_host.restype = C.c_int
    L.sxs_label_pick_host.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, u64p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
                                      C.c_void_p, C.c_uint64, u64p, u64p, u64p]
    L.sxs_guarded.restype, L.sxs_guarded.argtypes = C.c_void_p, [C.c_uint64, C.POINTER(C.c_void_p), u64p]
    L.sxs_unmap.restype, L.sxs_unmap.argtypes = None, [C.c_void_p, C.c_uint64]
    return L


@pytest.fixture(scope="module")
def selre():
    """the regex set's builder, for its codes and texts"""
    L = C.CDLL(tsc.built("libselre_core_host.so", "selre_core_host.cpp", ["-O2", "-fPIC", "-shared"]))
    L.sxs_selre_create.restype = C.c_void_p
    L.sxs_selre_create.argtypes = [C.POINTER(sx.Pattern), C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.c_char_p, C.c_uint32]
    L.sxs_selre_free.restype, L.sxs_selre_free.argtypes = None, [C.c_void_p]
    return L


def want_labels(patterns, nocase, strings):
    """Python's re.search per pattern: bit p of string i's label"""
    res = [re.compile(to_python(p), re.IGNORECASE if nocase else 0) for p in patterns]
    return [sum(1 << p for p, r in enumerate(res) if r.search(s) is not None) for s in strings]


def create(L, pats, n=None, flags=0):
    """(handle or None, label_build's code, its text) for (bytes, len) pairs"""
    arr = (sx.Pattern * max(1, len(pats)))(*[sx.Pattern(p, ln) for p, ln in pats])
    rc, err = C.c_int(99), C.create_string_buffer(512)
    h = L.sxs_label_create(arr, len(pats) if n is None else n, flags, C.byref(rc), err, 512)
    assert bool(h) == (rc.value == sx.SX_OK)
    return h, rc.value, err.value.decode(errors="replace")


def create_rc(L, pats, n=None, flags=0):
    h, rc, err = create(L, pats, n, flags)
    if h:
        L.sxs_label_free(h)
    return rc, err


class HostLabels:
    """a set as the builder makes it; .info: sx_label_set_info's fields plus here_first, dead, root_here, all"""

    def __init__(self, L, patterns, nocase=False):
        self.L, self.patterns, self.nocase = L, [bytes(p) for p in patterns], nocase
        self.h, rc, err = create(L, [(p, len(p)) for p in self.patterns], flags=NOCASE if nocase else 0)
        assert rc == sx.SX_OK and self.h, (rc, err, self.patterns)
        i, shape = sx.LabelSetInfo(), (C.c_uint64 * 6)()
        L.sxs_label_info(self.h, C.byref(i), shape)
        self.info = dict({k: getattr(i, k) for k, _ in sx.LabelSetInfo._fields_}, here_first=shape[0], dead=shape[1], root_here=shape[2], all=shape[3])
        # what the header promises of every set
        f, n = self.info, len(self.patterns)
        assert f["n_patterns"] == n and f["nocase"] == int(nocase) and f["all"] == (1 << n) - 1 and f["root_here"] & ~f["all"] == 0
        assert 1 <= f["classes"] <= 256 and 1 <= f["states"] <= sx.SX_SELECT_REGEX_MAX_STATES
        assert f["lds_states"] == min(f["states"], 48 * 1024 // (f["classes"] * 2)) and f["lds_states"] * f["classes"] * 2 <= 48 * 1024
        assert 1 <= f["here_first"] <= f["states"] and shape[4] == f["here_states"] == f["states"] - f["here_first"] and shape[5] == f["states"]
        assert f["table_bytes"] == 256 + f["states"] * f["classes"] * 2 + f["here_states"] * 8 + f["states"] * 8
        assert f["dead"] in (NONE, f["states"] - 1)

    def free(self):
        self.L.sxs_label_free(self.h)
        self.h = None


class Counters:
    """the set's counters as sx_label_set_reset leaves them, and Python's count next to them"""

    def __init__(self, n_patterns):
        self.n = n_patterns
        self.findings, self.first = (C.c_uint64 * 64)(), (C.c_uint64 * 64)(*([NEVER] * 64))
        self.want_findings, self.want_first = [0] * 64, [NEVER] * 64

    def expect(self, labels, ordinal):
        for i, lab in enumerate(labels):
            for p in range(64):
                if lab >> p & 1:
                    self.want_findings[p] += 1
                    self.want_first[p] = min(self.want_first[p], ordinal + i)

    def check(self):
        assert list(self.findings) == self.want_findings and list(self.first) == self.want_first, \
            (list(self.findings)[:self.n], self.want_findings[:self.n], list(self.first)[:self.n], self.want_first[:self.n])


def label_set(L, hs, strings, packed=True, layout="packed", rng=None, ordinal=0, groups=2, counters=None, want=None, lens=None):
    """hs over `strings` laid out as `layout`, against Python's re per pattern; returns (the labels, steps outside "LDS", all steps).
    lens: the records' str_len where they are to differ from the strings' lengths (the early exit)."""
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
        for i, ln in (lens or {}).items():
            arr[i].str_len = ln
        expect = want_labels(hs.patterns, hs.nocase, strings)
        if want is not None:
            assert expect == list(want), (hs.patterns, expect, list(want))     # (the case is what its author meant)
        counters = counters or Counters(len(hs.patterns))
        counters.expect(expect, ordinal)
        got = (C.c_uint64 * max(1, n))(*([0xEEEEEEEEEEEEEEEE] * max(1, n)))
        far_steps, steps = C.c_uint64(), C.c_uint64()
        rc = L.sxs_label_host(hs.h, C.addressof(arr), n, int(packed), base, ordinal, groups, got, counters.findings, counters.first,
                              C.byref(far_steps), C.byref(steps))
        assert rc == 0, rc
        got = list(got)[:n]
        assert got == expect, (hs.patterns, hs.nocase, [(i, strings[i], hex(got[i]), hex(expect[i])) for i in range(n) if got[i] != expect[i]][:5])
        counters.check()
        assert steps.value <= sum(len(s) for s in strings)
        return got, far_steps.value, steps.value
    finally:
        L.sxs_unmap(region, region_bytes)


def check(L, strings, patterns, nocase=False, want=None, every=True, **kw):
    """one set over both record types and both layouts (every=False: packed records, back to back, only)"""
    if isinstance(patterns, bytes):
        patterns = [patterns]
    hs = HostLabels(L, patterns, nocase)
    try:
        got = None
        for packed in ((True, False) if every else (True,)):
            for layout in (("packed", "scattered") if every else ("packed",)):
                for groups in ((1, 3) if every else (2,)):
                    got, _, _ = label_set(L, hs, strings, packed, layout, want=want, groups=groups, **kw)
        return got
    finally:
        hs.free()


# ---- 1. refusals and limits: the regex set's, code and text

def both(core, selre, pats, n=None, flags=0):
    """label_build's (code, text), which must be selre_build's"""
    arr = (sx.Pattern * max(1, len(pats)))(*[sx.Pattern(p, ln) for p, ln in pats])
    rc, err = C.c_int(99), C.create_string_buffer(512)
    h = selre.sxs_selre_create(arr, len(pats) if n is None else n, flags, C.byref(rc), err, 512)
    if h:
        selre.sxs_selre_free(h)
    got = create_rc(core, pats, n, flags)
    assert got == (rc.value, err.value.decode(errors="replace")), (pats[:2], got, rc.value, err.value)
    return got


def test_every_refusal_and_limit_of_the_regex_set_gives_the_same_code_and_text(core, selre):
    bad, ok = sx.SX_E_INVALID, sx.SX_OK
    for p, off in REFUSED:
        rc, err = both(core, selre, [(p, len(p))])
        assert rc == bad and "pattern 0, offset %d:" % off in err, (p, rc, err)
        rc, err = both(core, selre, [(b"ok", 2), (b"a|b", 3), (p, len(p))], flags=NOCASE)
        assert rc == bad and "pattern 2, offset %d:" % off in err, (p, rc, err)
    for p in (b"a{255}", b"a{0,255}", b"}", b"]", b"a|", b"|", b"()", b"(|)", b"\\{1\\}", b"[{]", b"a{,3}", b"-", b"[a-]", b"(?:)"):
        assert both(core, selre, [(p, len(p))])[0] == ok, p
    rc, err = both(core, selre, [(b"^[ab]*a[ab]{16}$", 16)])
    assert rc == bad and "SX_SELECT_REGEX_MAX_STATES" in err
    for p in (b"((a{255}){255}){255}", b"(((){255}){255}){255}"):
        rc, err = both(core, selre, [(p, len(p))])
        assert rc == bad and "SX_SELECT_REGEX_MAX_POSITIONS" in err
    p = b"^(a{255}){200}"
    rc, err = both(core, selre, [(p, len(p))] * 2)
    assert rc == bad and "pattern 1" in err and "SX_SELECT_REGEX_MAX_POSITIONS" in err
    many = [(b"ab", 2)] * 65
    assert both(core, selre, many, n=0)[0] == bad and both(core, selre, many, n=64)[0] == ok
    rc, err = both(core, selre, many, n=65)
    assert rc == bad and "n_patterns" in err
    long_one = b"q" * 1025
    assert both(core, selre, [(long_one, 0)])[0] == bad and both(core, selre, [(long_one, 1024)])[0] == ok
    rc, err = both(core, selre, [(b"ok", 2), (long_one, 1025)])
    assert rc == bad and "pattern 1" in err
    for p, word in ((b"a{256}", "SX_SELECT_REGEX_MAX_REPEAT"), (b"a{3,2}", "m > n")):
        rc, err = both(core, selre, [(p, len(p))])
        assert rc == bad and word in err
    assert both(core, selre, [(None, 3)])[0] == bad and both(core, selre, [(b"ok", 2), (None, 1)])[0] == bad
    rc, err = C.c_int(99), C.create_string_buffer(64)
    assert core.sxs_label_create(None, 1, 0, C.byref(rc), err, 64) is None and rc.value == bad
    assert both(core, selre, [(b"a", 1)], flags=NOCASE)[0] == ok
    for flags in (sx.SX_SELECT_INVERT, 4, NOCASE | 1 << 31):
        assert both(core, selre, [(b"a", 1)], flags=flags)[0] == bad
    for p, compiles in DEEP:
        assert (both(core, selre, [(p, len(p))])[0] == ok) == compiles


def test_a_label_set_meets_the_state_limit_sooner_than_a_regex_set(core, selre):
    """nothing absorbs: next to the literal b, [ab]*a[ab]{17} keeps its 2^17 subsets apart, which the regex set never makes because
    its walk is in `matched` behind the first b"""
    pats = [(b"[ab]*a[ab]{17}", 14), (b"b", 1)]
    arr = (sx.Pattern * 2)(*[sx.Pattern(p, ln) for p, ln in pats])
    rc, err = C.c_int(99), C.create_string_buffer(512)
    h = selre.sxs_selre_create(arr, 2, 0, C.byref(rc), err, 512)
    assert h and rc.value == sx.SX_OK          # "some pattern matches": b alone decides nearly everything
    selre.sxs_selre_free(h)
    rc, err = create_rc(core, pats)
    assert rc == sx.SX_E_INVALID and err == "the patterns need more than SX_SELECT_REGEX_MAX_STATES (65536) states"


# sha256 of sxs_label_table's bytes — LabelTable's seven words and two masks, the class map, then next, here and end — of
# test_selre_core.PINNED_SETS, in its order, as commit 046f17a gave them, the last one in which label_build had a subset construction,
# a numbering and a row writer of its own: its output has not changed by a bit
LABEL_PINNED = [
    "843e8070bd2a1c40f17162d81702a39387431604fb9f5b00bb2ec046ff92b7b1", "98c492ea8b412e2d9c1fd509caa1a40fd0a98f9f6273aac1a5855088ed61830a",
    "b20fcefad92041b14210e439436e1a38b5241d4767eb67eaaee385a406beec9a", "49d26f4639f9717ca2e03798354cb9ac6e837c517d7dc147149d371363cb7569",
    "3abba6a11f856b9e68458a2dcdeaff1aa8415e5764f255addc2476d0bdfbd048", "fd82138b83f1d8570f957db8c89acdad11ad4694b610df73288087905f200334",
    "67a09ac27e79ef4d6f2d951f2e5990618bd68b6c5e56fe47444ebd2e88807793", "178da0314ce9bf6299d78303974c9b76d662d043cf631634a5429ee4e6f90d10",
    "139ca1494b714f45aa7e06999fce1afe0dc2288956f410ba68fafe7db1d838fa", "a021fba1ed861323b26a5ee1fff2ba1d199b6f646956b70e4c3cdf2200304e86",
    "002ac128e1e302ed3f30eb9c0af8b78a04442e03edbf71bb7e450a24c2f9c92b", "4a9f282687211f4a3392752e159a8dd45c550afee373d39bcc507ad6c236b5c6",
    "a392f2f825ea9e0305eec6efb1f89e00401b1ba8f46bdc12f8d4fa7aa50878c9", "49df8df0fc0d22a52e0e6e512ca78e8e4c53a0aec12122ce64064718dc9c978f",
    "e2e96e4abc15852616373fd4ae38544509b1da0b9cf46fc5ee2c905bf875b000", "c2df9bdfe0bd7a0baa06d8f140cb585510c7bc20538fc3a01cc864224d2a379a",
    "2203674b158f6fd8ad1f4703373bb5a55a4ad6a39edb92f3ed7b8380fb2b5734",
]


def test_the_label_sets_tables_are_unchanged(core):
    assert len(LABEL_PINNED) == len(PINNED_SETS)
    shapes, most_pairs = set(), 0
    for (pats, flags), digest in zip(PINNED_SETS, LABEL_PINNED):
        hs = HostLabels(core, pats, flags == NOCASE)
        f = hs.info
        buf = C.create_string_buffer(28 + 16 + f["table_bytes"])
        assert core.sxs_label_table(hs.h, buf, len(buf)) == len(buf) and core.sxs_label_table(hs.h, buf, len(buf) - 1) == 0
        assert hashlib.sha256(buf.raw).hexdigest() == digest, pats
        words = [int.from_bytes(buf.raw[k:k + 8], "little") for k in range(28 + 16 + 256 + f["states"] * f["classes"] * 2, len(buf), 8)]
        here, end = [0] * f["here_first"] + words[:f["here_states"]], words[f["here_states"]:]
        most_pairs = max(most_pairs, len(set(zip(here, end))))
        shapes.add((f["states"] == 1, f["dead"] != NONE, f["here_states"] > (f["dead"] != NONE), f["root_here"] != 0, f["all"] == 2 ** 64 - 1))
        hs.free()
    # every branch of the numbering is among them: `dead` as the only state, as the last one and not at all, states with here != 0, a
    # root with a `here` of its own, 64 patterns; and more pairs of masks than a byte could number
    assert (True, True) in {s[:2] for s in shapes} and all({True, False} <= {s[k] for s in shapes if not s[0]} for k in (1, 2, 3, 4)), shapes
    assert most_pairs > 256, most_pairs


# ---- 2. hand-written cases

def test_the_empty_string_is_decided_by_the_root(core):
    strings = [b"", b"a", b"b", b"", b"aa"]
    check(core, strings, b"a*", want=[1, 1, 1, 1, 1])
    check(core, strings, b"^$", want=[1, 0, 0, 1, 0])
    check(core, strings, b"^", want=[1, 1, 1, 1, 1])
    check(core, strings, b"$", want=[1, 1, 1, 1, 1])
    check(core, strings, [b"a*", b"^$", b"^", b"$", b"x", b"b$"], want=[15, 13, 45, 15, 13])
    check(core, [b""] * 65, [b"^$", b"a"], want=[1] * 65)
    # a*, ^: every bit from the start, no byte is read; ^$: the first byte leads to `dead`; $ and x walk every byte
    for p, root_here, states, want_steps in ((b"a*", 1, 1, 0), (b"^", 1, 2, 0), (b"$", 0, 1, 4), (b"^$", 0, 2, 3), (b"x", 0, 2, 4)):
        hs = HostLabels(core, [p])
        assert (hs.info["root_here"], hs.info["states"]) == (root_here, states), (p, hs.info)
        _, _, steps = label_set(core, hs, strings)
        assert steps == want_steps, (p, steps)
        hs.free()


def test_here_and_end_disagree_where_one_pattern_is_anchored_at_each_end(core):
    strings = [b"abc", b"xabc", b"abcx", b"ac", b"bc", b"xbc", b"c", b"", b"ab", b"cab", b"abab"]
    check(core, strings, [b"^ab", b"bc$"], want=[3, 2, 1, 0, 2, 2, 0, 0, 1, 0, 1])
    check(core, strings, [b"bc$", b"^ab"], want=[3, 1, 2, 0, 1, 1, 0, 0, 2, 0, 2])
    check(core, strings, [b"c$", b"c"], want=[3, 3, 2, 3, 3, 3, 3, 0, 0, 2, 0])          # the same byte: `here` has bit 1, `end` bit 0
    check(core, strings, [b"^a", b"b$", b"^$", b"a.*c", b"(^x|b)c"], want=[25, 24, 25, 9, 16, 16, 0, 4, 3, 2, 3])
    # no "in front of a trailing newline" rule, and a match never spans two records
    check(core, [b"ab\n", b"ab", b"\nab", b"....ab", b"cd...."], [b"ab$", b"^ab", b"abcd", b"^cd"], want=[2, 3, 1, 1, 8])
    hs = HostLabels(core, [b"^ab", b"bc$"])
    assert hs.info["dead"] == NONE and hs.info["here_states"] >= 1        # bc$ can begin anywhere: nothing is dead
    hs.free()


def test_64_patterns_and_bit_63_alone(core):
    pats = [b"k%02d;" % p for p in range(63)] + [b"^z+$"]
    strings = [b"zz", b"k05;k62;", b"z", b"", b"k00;" + b"z", b"k62;", b"zzk"] + [b"k%02d;" % p for p in range(63)]
    want = [1 << 63, 1 << 5 | 1 << 62, 1 << 63, 0, 1, 1 << 62, 0] + [1 << p for p in range(63)]
    got = check(core, strings, pats, want=want)
    assert got[0] == 0x8000000000000000 and got[2] == 0x8000000000000000
    hs = HostLabels(core, pats)
    assert hs.info["all"] == 0xFFFFFFFFFFFFFFFF
    c = Counters(64)
    label_set(core, hs, strings, counters=c, ordinal=1 << 40)
    assert c.findings[63] == 2 and c.first[63] == 1 << 40 and c.findings[62] == 3 and c.first[62] == (1 << 40) + 1
    hs.free()


def test_a_set_that_reaches_dead(core):
    strings = [b"x" + b"a" * 500, b"abc" + b"y" * 500, b"ab" + b"y" * 500, b"abd"]
    hs = HostLabels(core, [b"^abc", b"^abd$"])
    assert hs.info["dead"] == hs.info["states"] - 1
    _, _, steps = label_set(core, hs, strings, want=[0, 1, 0, 2])
    assert steps == 1 + 4 + 3 + 3          # a mismatch; abc and one byte more, which ends ^abd$; the mismatch at the third byte; the string
    hs.free()
    hs = HostLabels(core, [b"a^b"])
    assert hs.info["states"] == 1 and hs.info["dead"] == 0
    _, _, steps = label_set(core, hs, strings, want=[0, 0, 0, 0])
    assert steps == 0
    hs.free()
    hs = HostLabels(core, [b"^abc", b"c"])
    assert hs.info["dead"] == NONE
    hs.free()


def test_the_all_bits_early_exit_reads_no_further(core):
    """every pattern has matched before the last byte: the lane stops there.  The last record claims more bytes than the arena has in
    front of the page without access; the walk would fault on the first of them."""
    hs = HostLabels(core, [b"ab", b"^x", b"b+c"])
    strings = [b"xabbc" + b"q" * 40, b"xab" + b"q" * 40, b"xabc"]
    _, _, steps = label_set(core, hs, strings, want=[7, 3, 7], lens={2: 4 + 100})
    assert steps == 5 + 43 + 4 and steps < sum(len(s) for s in strings)
    hs.free()
    hs = HostLabels(core, [b"a"])            # a one-pattern set stops where the regex selection stops
    _, _, steps = label_set(core, hs, [b"qqa" + b"q" * 100, b"a"], want=[1, 1], lens={1: 50})
    assert steps == 3 + 1
    hs.free()


def test_the_fold_is_re_ignorecase_on_a_bytes_pattern(core):
    strings = [b"z", b"A", b"a", b"Z", b"[", b"`", b"_", b"m", b"M", b"\xc3\x84", b"\xc3\xa4", b"MiXeD", b"mixed"]
    pats = [b"^[Z-a]$", b"^m$", b"^M$", b"[^m]", b"^\xc3\x84$", b"^mIxEd$"]
    folded = check(core, strings, pats, nocase=True)
    plain = check(core, strings, pats)
    assert folded[0] & 1 and not plain[0] & 1 and folded[7] & 6 == 6 and plain[7] & 6 == 2 and folded[9] & 16 and not folded[10] & 16
    assert folded[11] & 32 and folded[12] & 32 and not plain[11] & 32


def test_rows_in_lds_and_rows_in_the_table(core):
    rng = random.Random(4800)
    words = [text(rng, 12, b"abcdefghijklmnopqrstuvwxyz") for _ in range(400)]
    pats = [b"|".join(words[k:k + 40]) for k in range(0, 400, 40)]
    hs = HostLabels(core, pats)
    assert hs.info["states"] > hs.info["lds_states"] > 0 and hs.info["classes"] == 27, hs.info
    strings = [text(rng, rng.randrange(0, 60), b"abcdefghijklmnopqrstuvwxyz") for _ in range(600)]
    for k in range(0, 600, 3):
        for _ in range(rng.randrange(1, 3)):
            at = rng.randrange(0, len(strings[k]) + 1)
            strings[k] = strings[k][:at] + words[rng.randrange(400)][:rng.choice((12, 12, 11, 8))] + strings[k][at:]
    for packed, layout in ((True, "packed"), (False, "scattered")):
        got, far, _ = label_set(core, hs, strings, packed, layout, rng=rng, groups=3)
        assert far > 0 and len({g for g in got}) > 10 and any(bin(g).count("1") == 2 for g in got)
    hs.free()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200, 1100])
def test_record_counts_around_a_wavefront_and_a_workgroup(core, n):
    rng = random.Random(70 + n)
    strings = [text(rng, rng.randrange(0, 24), b"abc") for _ in range(n)]
    strings[-1] = b"the last one"
    hs = HostLabels(core, [b"ab+c|^c", b"one$", b"^$", b"#"])
    for packed in (True, False):
        for groups in (1, 2, 5):
            got, _, _ = label_set(core, hs, strings, packed, "scattered" if packed else "packed", rng=rng, groups=groups, ordinal=77)
            assert got[-1] == 2 and all(g & 8 == 0 for g in got)
    hs.free()


# ---- 3. random cases

def random_case(rng):
    """(patterns, nocase, strings) over a 2- or 3-letter alphabet, 1..8 patterns"""
    alphabet = rng.choice((b"ab", b"abc", b"aB", b"abC"))
    trees = [Tree(rng, alphabet, rng.randrange(0, 4)) for _ in range(rng.randrange(1, 9))]
    pats = [t.render() for t in trees]
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
    return pats, rng.random() < 0.3, strings


def test_2000_random_cases(core):
    rng = random.Random(2064)
    seen_set, seen_clear = [0] * 8, [0] * 8
    for case in range(2000):
        pats, nocase, strings = random_case(rng)
        hs = HostLabels(core, pats, nocase)         # (a refused case fails here: the generator stays inside the language and the limits)
        try:
            got, _, _ = label_set(core, hs, strings, rng.random() < 0.5, rng.choice(("packed", "scattered")), rng=rng, groups=rng.randrange(1, 4),
                                  ordinal=rng.randrange(1 << 33))
            for lab in want_labels(pats, nocase, strings):          # the reference alone: every case can fail
                for p in range(len(pats)):
                    if lab >> p & 1:
                        seen_set[p] += 1
                    else:
                        seen_clear[p] += 1
        finally:
            hs.free()
    assert min(seen_set) > 500 and min(seen_clear) > 500, (seen_set, seen_clear)      # every pattern position decides something, both ways


# ---- 4. the counters over two buffers of one stream

def test_counters_over_two_buffers_with_an_ordinal_base(core):
    rng = random.Random(12)
    pats = [b"ab", b"^c", b"c$", b"bbb", b"^$", b"zz"]
    hs = HostLabels(core, pats)
    one = [text(rng, rng.randrange(0, 12), b"abc") for _ in range(300)]
    two = [text(rng, rng.randrange(0, 12), b"abc") for _ in range(150)] + [b"bbb", b"", b"zz!"]
    one = [s for s in one if b"bbb" not in s and s]            # `bbb` and `^$` first occur in the second buffer, `zz` last of all
    two[:150] = [s for s in two[:150] if b"bbb" not in s and s] + [b"a"] * (150 - len([s for s in two[:150] if b"bbb" not in s and s]))
    c = Counters(len(pats))
    label_set(core, hs, one, counters=c, ordinal=0, groups=3)
    label_set(core, hs, two, packed=False, layout="scattered", counters=c, ordinal=len(one), groups=2)
    assert c.first[3] == len(one) + 150 and c.first[4] == len(one) + 151 and c.first[5] == len(one) + 152
    assert list(c.findings)[3:6] == [1, 1, 1] and c.findings[0] > 50 and c.first[0] < 20
    assert list(c.findings)[6:] == [0] * 58 and list(c.first)[6:] == [NEVER] * 58
    hs.free()


# ---- 5. the selection by label

def picked(label, any_, all_, none):
    return (any_ == 0 or label & any_ != 0) and label & all_ == all_ and label & none == 0


@pytest.mark.parametrize("packed", [True, False])
def test_the_pick_predicate_and_what_pass_two_makes_of_it(core, packed):
    rng = random.Random(640 + packed)
    top = 1 << 63
    for n in (1, 64, 65, 300):
        strings = [text(rng, rng.randrange(0, 20), b"abcdef") for _ in range(n)]
        labels = [rng.choice((0, 1, 2, 3, 5, 6, 7, top, top | 1, rng.getrandbits(64))) for _ in range(n)]     # made by Python
        layout = rng.choice(("packed", "scattered"))
        offs, arena = lay_out(strings, layout, rng)
        region, region_bytes = C.c_void_p(), C.c_uint64()
        base = core.sxs_guarded(max(1, len(arena)), C.byref(region), C.byref(region_bytes))
        try:
            C.memmove(base, arena, len(arena))
            arr = records(strings, offs, packed)
            lab = (C.c_uint64 * n)(*labels)
            masks = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (6, 0, 0), (0, 6, 0), (0, 0, 6), (3, 4, 0), (7, 1, 2), (top, 0, 0), (0, top, 0),
                     (0, 0, top), (0, top | 1, 0), (1 << 40, 0, 0), (0, 0, (1 << 64) - 1), (0, (1 << 64) - 1, 0)]
            masks += [(rng.getrandbits(64) & rng.getrandbits(64), rng.getrandbits(64) & rng.getrandbits(64) & rng.getrandbits(64),
                       rng.getrandbits(64) & rng.getrandbits(64) & rng.getrandbits(64)) for _ in range(8)]
            for any_, all_, none in masks:
                want = [i for i in range(n) if picked(labels[i], any_, all_, none)]
                total = sum(len(strings[i]) for i in want)
                out = ((sx.Finding16 if packed else sx.Finding) * n)()
                raw = C.create_string_buffer(b"\xEE" * (total + 64), total + 64)
                waves = (n + 63) // 64
                wm = (C.c_uint64 * (waves + 1))()
                n_sel, sel_bytes = C.c_uint64(), C.c_uint64()
                rc = core.sxs_label_pick_host(C.addressof(arr), n, int(packed), base, lab, any_, all_, none, C.addressof(out), C.addressof(raw), total,
                                              wm, C.byref(n_sel), C.byref(sel_bytes))
                assert rc == 0, rc
                got = [w * 64 + b for w in range(waves) for b in range(64) if wm[w] >> b & 1]
                assert got == want, (hex(any_), hex(all_), hex(none), got[:5], want[:5])
                assert (n_sel.value, sel_bytes.value) == (len(want), total)
                out_arena, off = raw.raw, 0
                assert out_arena[total:] == b"\xEE" * 64
                for k, i in enumerate(want):
                    assert fields(out[k], packed) == fields(arr[i], packed) and out[k].str_off == off
                    assert out_arena[off:off + len(strings[i])] == strings[i]
                    off += len(strings[i])
            if n == 300:
                assert 0 < len([i for i in range(n) if picked(labels[i], 3, 4, 0)]) < n
        finally:
            core.sxs_unmap(region, region_bytes)


# ---- 6. the builder and the core under the address and undefined-behaviour sanitizers, as a program of their own

def test_a_sanitizer_build_refuses_and_labels_the_same(tmp_path):
    exe = built("label_build_main", "label_build_main.cpp", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    rng = random.Random(364)
    cases = []      # (patterns, flags, strings, want: a code or the labels)
    for p, _ in REFUSED:
        cases.append(([p], 0, [b"a"], sx.SX_E_INVALID))
    for pats in ([b"ab"] * 65, [b"q" * 1025], [b"a{256}"], [b"a{3,2}"], [b"^[ab]*a[ab]{16}$"], [b"((a{255}){255}){255}"], [b""]):
        cases.append((pats, 0, [b"a"], sx.SX_E_INVALID))
    cases.append(([b"a"], 4, [b"a"], sx.SX_E_INVALID))
    for p, compiles in DEEP:
        strings = [b"", b"a", b"b", b"aaa", b"ba", b"xaby", b"abab"]
        cases.append(([p], 0, strings, want_labels([p], False, strings) if compiles else sx.SX_E_INVALID))
    pats = [b"k%02d;" % p for p in range(63)] + [b"^z+$"]
    strings = [b"zz", b"k05;k62;", b""] + [b"k%02d;" % p for p in range(0, 63, 9)]
    cases.append((pats, 0, strings, want_labels(pats, False, strings)))
    for _ in range(300):
        pats, nocase, strings = random_case(rng)
        cases.append((pats, NOCASE if nocase else 0, strings, want_labels(pats, nocase, strings)))
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for pats, flags, strings, _ in cases:
            f.write("case %d\n" % flags)
            f.writelines("p %s\n" % p.hex() for p in pats)
            f.writelines("s %s\n" % s.hex() for s in strings)
            f.write("end\n")
    run = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-3000:]
    lines = iter(run.stdout.splitlines())
    for pats, flags, strings, want in cases:
        line = next(lines)
        if isinstance(want, int):
            assert line.startswith("rc %d " % want), (pats, line)
            continue
        assert line.split() == ["lab"] + ["%x" % w for w in want], (pats, flags, line, want)
        counts = ["%d:%d" % (sum(w >> p & 1 for w in want), min([1000 + i for i, w in enumerate(want) if w >> p & 1], default=NEVER)) for p in range(len(pats))]
        assert next(lines).split() == ["cnt"] + counts, (pats, flags)
    assert next(lines, None) is None
