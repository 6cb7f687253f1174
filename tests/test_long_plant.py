"""tests/long_plant.py against the oracle: conditions on the INPUTS of tests/test_gpu_result_long_strings.py, asserted on the oracle's
strings — no product code runs here, except where the last tests feed the same strings to the lane-function harnesses of the order,
the substring selection and the extraction (as tests/test_order_core.py, tests/test_select_core.py and tests/test_extract_core.py
drive them: plain host C++, the arena in front of a page without access)."""
import collections
import re

import pytest

import long_plant as lp
import refconfig as rc
import result_plant as rp
import test_extract_core as xc
import test_order_core as oc
import test_select_core as sc
from test_extract_core import core as extract_core      # (the harnesses' fixtures, under names of their own)
from test_order_core import core as order_core, fold, lcp
from test_select_core import core as select_core
import test_label_core as lc
import test_selre_core as rx
import test_selset_core as ks
import test_seltally_core as tc
from test_label_core import core as label_core
from test_selre_core import core as selre_core
from test_selset_core import core as selset_core
from test_seltally_core import core as seltally_core


@pytest.fixture(scope="module")
def two():
    """the oracle's rows of the two-Mission source, and the strings of its first Mission"""
    e = rp.expected(lp.msl2(), lp.buffer(lp.lines()))
    return e, [s for s, m in zip(e.strs, e.mission.tolist()) if m == 0]


@pytest.fixture(scope="module")
def one():
    return rp.expected(lp.msl1(), lp.buffer(lp.one_lines()))


@pytest.fixture(scope="module")
def wave():
    return rp.expected(lp.msw(), lp.buffer(lp.wave_lines()))


def test_the_oracle_returns_every_line_whole(two, one, wave):
    e, first = two
    ls = lp.lines()
    assert 1000 <= len(ls) <= 5000 and len(lp.buffer(ls)) < 1 << 19                 # a few thousand findings, well under 1 MiB
    assert e.n == 2 * len(ls) and {r[2] for r in e.rows} == {b"(a ascii)", b"(b UTF-8)"}
    for m in (0, 1):
        assert [s for s, x in zip(e.strs, e.mission.tolist()) if x == m] == ls      # found once by each Mission, no line cut
    assert not e.completes.any() and first == ls
    assert one.strs == lp.one_lines() and set(lp.utf8_lines()) <= set(one.strs)      # (a line behind one of 255 characters counts as its continuation: whole all the same)
    assert wave.strs == lp.wave_lines() and not wave.completes.any()
    assert max(len(s.decode()) for s in wave.strs) == 64 and max(len(s) for s in wave.strs) == 256 and sum(1 for s in wave.strs if len(s) >= 192) > 50
    assert max(len(s) for s in one.strs) > 970 and max(len(s.decode()) for s in one.strs) == 255
    assert lp.lines() == ls and lp.prefix(40) == lp.buffer(ls[:40])                   # the same lines, whatever was asked first


def test_the_lengths(two):
    _, strs = two
    lengths = {len(s) for s in strs}
    assert lengths >= set(lp.LENGTHS) and max(lengths) == 1024 and min(lengths) == 7
    assert {n % 16 for n in lengths} == set(range(16))
    assert sum(1 for s in strs if len(s) > 64) > 250 and sum(1 for s in strs if len(s) >= 1000) > 30


def parting(strs):
    """{the byte at which two different strings first differ, both being longer than that}"""
    ks = sorted(set(strs))
    return {lcp(a, b) for a, b in zip(ks, ks[1:]) if lcp(a, b) < min(len(a), len(b))}


def test_the_deep_families(two, one, wave):
    _, strs = two
    assert parting(strs) >= set(lp.STEMS) | {1023}                                    # ... and two lines of 1024 that differ in their last byte
    uniq = set(strs)
    for s in lp.STEMS:
        # a line that is a proper prefix of another, at a multiple of 8 bytes, in the family whose stem has s bytes
        cut = (s + 8) // 8 * 8
        assert any(len(a) == cut and any(b.startswith(a) and len(b) > cut for b in uniq) for a in uniq if len(a) == cut), s
    assert any(len(a) == 1016 and any(b.startswith(a) and len(b) == 1024 for b in uniq) for a in uniq)
    size = collections.Counter(s for s in strs if len(s) >= 256)
    assert {min(c, 3) for c in size.values()} == {1, 2, 3} and size[max(size, key=lambda s: (len(s), size[s]))] >= 3      # copies of a line of 1024
    folded = collections.Counter(fold(s) for s in strs if len(s) >= 256)
    assert len(folded) < len(size) and any(len(s) == 1024 and s != fold(s) and fold(s) in uniq for s in uniq)            # equal only under the fold
    # bytes >= 0x80 at a word's first and at its last byte, in the UTF-8 sources
    for e in (one, wave):
        assert any(len(s) > 8 and s[8] >= 0x80 for s in e.strs) and any(len(s) > 8 and s[7] >= 0x80 for s in e.strs)
        assert any(len(s) % 8 == 0 and s[-1] >= 0x80 for s in e.strs)
    assert parting(wave.strs) & set(range(240, 256)) and {216 * 2 // 1, 966} <= parting(one.strs) | {432} and 966 in parting(one.strs)                              # a stem of 60 four-byte characters; a Cyrillic one


@pytest.mark.parametrize("descending", [False, True], ids=["ascending", "descending"])
def test_the_rounds_leave_2_3_5_17_and_257_groups(two, descending):
    """a group key one bit too narrow merges two groups at 2^k + 1 of them"""
    e, _ = two
    left = lp.groups_left(e.strs, descending=descending)
    assert set(left) >= set(lp.GROUP_COUNTS), sorted(set(lp.GROUP_COUNTS) - set(left))
    assert len(left) == 1024 // 8 and left[-1] >= 2                                   # the last round, 128, still parts lines of 1024 bytes
    # the model is the rule: an item is undecided iff another shares its first 8 (d + 1) bytes
    for d in (0, 32, 80, 127):
        count = collections.Counter(s[:8 * d + 8] for s in e.strs if len(s) >= 8 * d + 8)
        assert left[d] == sum(1 for c in count.values() if c > 1)


def test_the_tokens_and_the_split_pairs(two, one, wave):
    e, strs = two
    assert lp.NEEDLE64[:1] + lp.NEEDLE64[-1:] == b"<>" and len(lp.NEEDLE64) == 64 and len(lp.KEYWORD255) == 255
    for tok in lp.TOKENS:
        n, h = len(tok), len(tok) // 2
        held = [s for s in strs if tok in s]
        assert any(s.startswith(tok) for s in held), tok                              # at offset 0
        assert any(len(s) == 1024 and s.endswith(tok) and s.count(tok) == 1 for s in held), tok      # the last bytes of a line of 1024
        deep = {s.find(tok) for s in held if len(s) == 1024}
        if n < 16:
            assert deep >= set(range(1000, 1016))                                     # one of them straddles a 16-byte boundary wherever it lies
        else:
            assert any(o + n > 1000 and o + n < 1024 for o in deep)                   # (longer than a chunk: it always straddles one)
        # split between the end of one finding and the beginning of the next, in the oracle's order: neither holds it
        pairs = [(a, b) for a, b in zip(e.strs, e.strs[1:]) if a.endswith(tok[:h]) and b.startswith(tok[h:])]
        assert pairs and all(tok not in a and tok not in b for a, b in pairs), tok
        assert all(tok in a + b for a, b in pairs)
    # the one-Mission source: behind byte 900 at sixteen neighbouring offsets, as the last bytes of a line, and split
    assert {s.find(lp.NEEDLE) for s in one.strs if len(s) > 900} >= set(range(910, 926)) and any(s.endswith(lp.NEEDLE) and len(s) > 970 for s in one.strs)
    assert any(s.startswith(lp.NEEDLE) for s in one.strs)
    assert sum(1 for a, b in zip(one.strs, one.strs[1:]) if a.endswith(lp.NEEDLE[:4]) and b.startswith(lp.NEEDLE[4:]) and lp.NEEDLE not in a and lp.NEEDLE not in b) >= 2
    h = len(lp.NEEDLE) // 2
    assert any(a.endswith(lp.NEEDLE[:h]) and b.startswith(lp.NEEDLE[h:]) and lp.NEEDLE not in a and lp.NEEDLE not in b for a, b in zip(wave.strs, wave.strs[1:]))
    assert any(s.startswith(lp.NEEDLE) for s in wave.strs) and any(s.endswith(lp.NEEDLE) and len(s) > 200 for s in wave.strs)


def test_the_dense_lines(two):
    _, strs = two
    rx = re.compile(b"|".join(lp.EXTRACTS))
    count = [len(rx.findall(s)) for s in strs]
    assert max(count) == 100 > 64 and strs[count.index(100)] == lp.DENSE              # more matches in one record than a wavefront has lanes
    assert [m for s in strs for m in rx.findall(s) if len(m) >= 1000] == [lp.ONE_MATCH] and lp.ONE_MATCH in strs
    assert sum(count) > len(strs) and count.count(0) > len(strs) // 10
    occ = rp.occurrences([lp.RUN], lp.TALLY)
    assert lp.RUN in strs and [occ[k].get(0, 0) for k in range(3)] == [599, 598, 600 - 254]      # overlapping places count


def test_every_pattern_decides_something(two):
    _, strs = two
    for r in lp.REGEXES + lp.LABELS:
        share = sum(1 for s in strs if rp.to_python(r).search(s))
        assert 0 < share < len(strs), r
    # one regex is anchored with `$`; another runs 1000 bytes and more of a line of 1024 before it fails or ends
    assert any(r.endswith(b"$") for r in lp.REGEXES)
    far = rp.to_python(lp.REGEXES[2])
    assert sum(1 for s in strs if far.search(s)) in range(1, 10) and sum(1 for s in strs if s.startswith(b"stem1000 ") and len(s) >= 1000 and not far.search(s)) > 20


def test_the_limit_source():
    ls = lp.limit_lines()
    e = rp.expected(lp.limit_ms(), lp.buffer(ls))
    for m in (0, 1):
        got = [s for s, x in zip(e.strs, e.mission.tolist()) if x == m]
        want = ls if m else [s for s in ls if max(s) < 0x80]                           # (the ASCII Mission finds no four-byte character)
        assert got == want, (m, [len(s) for s in got])
    assert not e.completes.any()
    assert {len(s) for s in e.strs} >= {16000, 64000} and max(len(s) for s in e.strs) == 64000 < 1 << 16
    assert [s for s in e.strs if lp.LIMIT_NEEDLE in s] == [ls[3]] * 2 and ls[7][:-8] == ls[3][:-8] and ls[7] != ls[3] and ls[3].endswith(lp.LIMIT_NEEDLE) and len(ls[3].decode()) == 16000
    assert e.strs.count(ls[1]) == 4 and ls[6][:-1] == ls[1][:-1] and ls[6] != ls[1]      # copies, and two lines that differ in their last byte


def test_expected_is_cached_by_every_field_of_every_mission():
    """two Mission lists that differ in -q alone have different findings"""
    data = b"abcdef\n" + b"0123456789" * 10 + b"\n"
    short = rp.expected(rc.missions(encodings=["ascii"], chars_min="4", output_line_len="64"), data)
    long_ = rp.expected(rc.missions(encodings=["ascii"], chars_min="4", output_line_len="1024"), data)
    assert [len(s) for s in short.strs] == [6, 64, 36] and [len(s) for s in long_.strs] == [6, 100]
    other = rp.expected(rc.missions(encodings=["ascii"], chars_min="10", output_line_len="64"), data)
    assert [len(s) for s in other.strs] == [64, 36]
    assert rp.expected(rc.missions(encodings=["ascii"], chars_min="4", output_line_len="64"), data) is short


# ---- the same strings through the lane-function harnesses: a failure on the device can be assigned to a lane function or to a kernel

def harness_strings():
    """a prefix of the plant's lines: deep families, the split needle, the dense lines and the long family's first members"""
    out = lp.lines()[:lp.HEAD]
    h = len(lp.NEEDLE) // 2
    assert any(a.endswith(lp.NEEDLE[:h]) and b.startswith(lp.NEEDLE[h:]) for a, b in zip(out, out[1:])) and lp.DENSE in out and lp.RUN in out
    assert parting(out) >= {23, 24, 25, 1000, 1023} and sum(1 for s in out if len(s) == 1024) >= 6
    return out


def test_the_order_core_over_the_long_lines(order_core):
    core = order_core
    strings = harness_strings()
    for flags in (0, oc.DESC, oc.NOCASE):
        _, info = oc.check(core, [strings[:70], strings[70:]], flags=flags, every=False)
        assert info["rounds"] == 1024 // 8 + 1 and info["tied"] >= 3
    oc.check(core, [strings], every=True, want_rounds=129)


def test_the_select_core_over_the_long_lines(select_core):
    core = select_core
    strings = harness_strings()
    for tok in (lp.NEEDLE, lp.NEEDLE64):
        for packed, layout in ((True, "packed"), (False, "scattered")):
            want, _ = sc.check(core, strings, [tok], packed, layout)
            assert len(want) >= 2 and all(tok in strings[i] for i in want)
        for misalign in (0, 5, 11):
            sc.check(core, strings, [tok], misalign=misalign)
    sc.check(core, strings, [lp.NEEDLE, b"tail3", b"77777"], flags=sc.INVERT)
    sc.check(core, strings, [lp.NEEDLE.upper()], flags=sc.NOCASE)
    sc.check(core, strings, [lp.NEEDLE.upper()], want_selected=[])


def test_the_extract_core_over_the_long_lines(extract_core):
    core = extract_core
    strings = harness_strings()
    rx = re.compile(b"|".join(lp.EXTRACTS))                  # runs of one class and a literal: leftmost-first is leftmost-longest
    expect = [[m.span() for m in rx.finditer(s)] for s in strings]
    assert max(len(m) for m in expect) == 100 and any(e - o >= 1000 for m in expect for o, e in m)
    hx = xc.HostExtract(core, lp.EXTRACTS)
    try:
        for packed, layout in ((True, "packed"), (False, "scattered")):
            xc.check_set(core, hx, strings, packed, layout, expect=expect)
    finally:
        hx.free()


def test_the_keyword_regex_label_and_tally_cores_over_the_long_lines(selset_core, selre_core, label_core, seltally_core):
    """the sets of the GPU tests compile, and the per-lane table walks give Python's answers on the same strings"""
    strings = harness_strings()
    want = ks.check(selset_core, strings, [lp.KEYWORD255, lp.NEEDLE, b"tail3", b"7" * 255], every=False)
    rx.check(selre_core, strings, lp.REGEXES, every=False)
    lc.check(label_core, strings, lp.LABELS, every=False)
    tc.check(seltally_core, strings, lp.TALLY, every=False)
    assert want is None or len(want) > 0
