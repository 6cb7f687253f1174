"""sx_result_fuzzy_device (Result.fuzzy_device): which keywords of a fuzzy set occur in every string of a result that lies in HBM within
their error budgets, decided on the device, and what the selections and the order make of the words.

The sources, over the lines of tests/fuzzy_plant.py (tests/test_fuzzy_plant.py asserts on the CPU what they hold: variants of the
planted words at 0 .. k + 1 errors at the head, in the middle and as the tail of a line, every bit both set and clear)
    wave k / lane k   one UTF-8 Mission — packed records on the wave path, unpacked ones on the lane-per-region replay —, k = 1, 63, 64,
                      65, 129; the first lines are a string of exactly len - k bytes and one a byte shorter
    merged            `-e ascii -e utf-8` under SX_MERGE_PART_FINDINGS=1024: several packed segments
    trip              R + 1 records in one segment, R = CUs x kRowsGroupsPerCu x kRowsWaves x 64 read from the sources as
                      tests/test_gpu_result_strides.py reads them: record R is the one record of the kernel's second trip, on the lane
                      that had record 0, which matched — and record R must not: a lane that kept its columns or its bits would say yes
    limit             long_plant.limit_lines(): 16 000 and 64 000 bytes, the match in the last eight bytes alone
and the output of a selection, of an extraction and of fold_device().  The sets (fuzzy_plant.SETS): one pattern; nine — the 32-bit words,
a group of eight and one more —; five — one pattern of 36 bytes: the 64-bit words, a group of four and one more —; sixty-four; a nocase
set; k = 0; and `many`, whose classes exceed the rows in LDS, with the planted words' letters among the rows read through L2.

Every expected word is fuzzy_plant.words() — Sellers' table in Python — of the oracle's string (result_plant.expected()); no value comes
from a product Scanner."""
import ctypes as C
import re

import numpy as np
import pytest

import fold_plant as fp
import fuzzy_plant as fz
import long_plant as lp
import stringsext_amd as sx
from test_gpu_fold_edges import PARTS, make_from
from test_gpu_measure_device import lying
from test_gpu_result_long_strings import check_sel
from test_gpu_result_strides import check_records, picked, printed_on_device, same, trip_sizes, words_of

pytestmark = pytest.mark.gpu

NEVER = sx.SX_LABEL_NEVER
SMALL = (1, 63, 64, 65, 129)

MAKERS = {
    "merged": lambda: make_from("merged", "merged", fp.ms2(), lp.buffer(fz.lines(fz.MERGED_LINES)), PARTS),
    "trip": lambda: make_from("trip", "wave", fp.ms1(), lp.buffer(fz.trip_lines(trip_sizes()[0]))),
    "limit": lambda: make_from("limit", "merged", lp.limit_ms(), lp.buffer(lp.limit_lines())),
}


@pytest.fixture(scope="module")
def sources():
    made = {}

    def get(name, k=None):
        if (name, k) not in made:
            made[name, k] = make_from("%s %d" % (name, k), name, fp.ms1(), lp.buffer(fz.lines(k))) if k else MAKERS[name]()
        return made[name, k]
    yield get
    for s in made.values():
        s.close()


def bit_counts(want, n_patterns, base):
    """(findings, first) per pattern from the words"""
    findings, first = [], []
    for p in range(n_patterns):
        has = np.nonzero((want >> np.uint64(p)) & np.uint64(1))[0]
        findings.append(len(has))
        first.append(base + int(has[0]) if len(has) else NEVER)
    return findings, first


def fuzzed(s, a_set, res=None, rows=None):
    """res.fuzzy_device() with a new set of a_set = (patterns, ks, nocase), checked: every word against the table, the host twin on every
    distinct string, the counters across two calls — the later buffer first: the minimum is taken —, reset(), the source byte for byte
    what it was, and a selection made before still printing what it printed.  Returns (the set, the Labels, the words)"""
    pats, ks, nocase = a_set
    res, rows = res or s.res, rows or s.rows
    before = lying(s.sc, res)
    head = rows.strs[0][:4]
    sel = res.select_device(head)
    text = printed_on_device(s.sc, sel)
    if rows.raw is not None:
        assert text == rows.take(rows.mask(lambda x: head in x)).text(), s.name
    fs = s.sc.fuzzy_set(pats, ks, ignore_case=nocase)
    info = fs.info
    assert (info.n_patterns, info.nocase, info.max_len, info.max_errors) == (len(pats), int(nocase), max(map(len, pats)), max(ks))
    assert fs.read() == ([0] * len(pats), [NEVER] * len(pats))
    want = fz.words(pats, ks, rows.strs, nocase)
    n = rows.n
    fs_f, fs_m = fs.counters_device()
    assert fs_f and fs_m and fs_f != fs_m
    res.fuzzy_device(fs, ordinal_base=n + 7).free()
    assert fs.read() == bit_counts(want, len(pats), n + 7), s.name
    lab = res.fuzzy_device(fs, ordinal_base=7)
    same(words_of(s.sc, lab, res), want, s.name + ": the words", rows.strs)
    findings, first = bit_counts(want, len(pats), 7)
    assert fs.read() == ([2 * f for f in findings], first), s.name
    assert np.frombuffer(s.sc.download(fs_f, 8 * len(pats)), dtype="<u8").tolist() == [2 * f for f in findings]
    for x in set(rows.strs):
        assert sx.fuzzy(pats, ks, x, nocase) == fz.word(pats, ks, x, nocase), (s.name, x[:60])
    fs.reset()
    assert fs.read() == ([0] * len(pats), [NEVER] * len(pats))
    assert lying(s.sc, res) == before, s.name
    assert printed_on_device(s.sc, sel) == text, s.name
    sel.free()
    return fs, lab, want


@pytest.mark.parametrize("k", SMALL)
@pytest.mark.parametrize("kind", ["wave", "lane"])
def test_the_words_of_one_mission_around_a_wavefront(sources, kind, k):
    s = sources(kind, k)
    assert s.rows.n == k and s.rows.strs == fz.lines(k)
    for name in ("one", "nine", "five"):
        fs, lab, want = fuzzed(s, fz.SETS[name])
        if k > 1:
            assert int(want[0]) & 1 == 1 and int(want[1]) & 1 == 0              # len - k bytes of the word; one byte fewer cannot match
            assert 0 < int((want != 0).sum()) < k
        lab.free(); fs.free()


@pytest.mark.parametrize("name", sorted(fz.SETS))
def test_the_words_of_merged_missions_in_several_segments_for_every_set(sources, name):
    s = sources("merged")
    assert len(s.res.device_segments()) >= 3
    fs, lab, want = fuzzed(s, fz.SETS[name])
    if name == "many":
        assert fs.info.lds_classes == 48 * 1024 // (64 * 8) < fs.info.classes and int(np.bitwise_or.reduce(want)) == 7
    else:
        assert fs.info.lds_classes == fs.info.classes
    if name == "sixty-four":
        assert 0 < int((want >> np.uint64(63)).sum()) < s.rows.n
    lab.free(); fs.free()


def test_one_record_in_the_second_trip_on_the_lane_that_had_a_match(sources):
    r = trip_sizes()[0]
    s = sources("trip")
    assert s.rows.n == r + 1 and len(s.res.device_segments()) == 1
    fs, lab, want = fuzzed(s, fz.SETS["one"])
    assert int(want[0]) == 1 and int(want[r]) == 0
    lab.free(); fs.free()
    fs, lab, want = fuzzed(s, fz.SETS["five"])
    assert int(want[0]) & 1 == 1 and int(want[r]) == 0
    lab.free(); fs.free()


def test_strings_of_16000_and_64000_bytes_with_the_match_in_their_last_bytes(sources):
    s = sources("limit")
    assert {16000, 64000} <= set(s.rows.length.tolist())
    pats, ks = fz.LONG_SET
    fs, lab, want = fuzzed(s, (pats, ks, False))
    long_ones = [int(w) for w, n in zip(want, s.rows.length) if n == 64000]
    assert len(long_ones) >= 3 and all(w & 9 for w in long_ones) and {w & 9 for w in long_ones} == {1, 8}
    lab.free(); fs.free()
    # the same in 64-bit words: a pattern of more than 32 bytes beside them
    fs, lab, want = fuzzed(s, (pats + [lp.limit_lines()[0] * 3], ks + [8], False))
    assert fs.info.max_len == 48
    lab.free(); fs.free()


# ---- other operations' outputs as the source

def test_the_output_of_a_selection_of_an_extraction_and_of_a_fold_as_the_source(sources):
    s = sources("merged")
    mask = s.rows.mask(lambda x: b"o" in x)
    assert 0 < mask.sum() < s.rows.n
    sel = s.res.select_device(b"o")
    fs, lab, _ = fuzzed(s, fz.SETS["nine"], sel, s.rows.take(mask))
    lab.free(); fs.free(); sel.free()
    # an extraction: the matches are the strings
    pattern = rb"[a-z0-9.#%&]{5,}"
    rx = re.compile(pattern)
    per_class = [rx.findall(u) for u in s.rows.uniq]
    count = np.array([len(m) for m in per_class], dtype=np.int64)[s.rows.inv]
    matches = [m for u in s.rows.inv.tolist() for m in per_class[u]]
    rows = s.rows.take(np.repeat(np.arange(s.rows.n), count), strs=matches)
    xs = s.sc.extract_set([pattern])
    ext = s.res.extract_device(xs)
    xs.free()
    check_records(s.sc, ext, rows, True, "the matches")
    fs, lab, want = fuzzed(s, fz.SETS["five"], ext, rows)
    assert 0 < int((want & np.uint64(1)).sum()) < rows.n
    lab.free(); fs.free(); ext.free()
    # a fold: its strings, and the answer carried back to the original strings
    fold = s.res.fold_device()
    pats, ks, _ = fz.SETS["nine"]
    folded = [sx.fold(p) for p in pats]
    assert folded[4] == pats[4] and folded[0] == pats[0]
    upper = ([p.decode().upper().encode() for p in pats], ks, False)      # 'ПАРОЛЬ', 'PASSWORD': in no line as they are
    assert int(np.bitwise_or.reduce(fz.words(upper[0], ks, s.rows.strs)) & np.uint64(1 << 4)) == 0
    fs, lab, want = fuzzed(s, ([sx.fold(p) for p in upper[0]], ks, False), fold, s.frows)
    bound = lab.rebind(s.res)
    pick = 1 << 4 | 1      # 'пароль' or 'password' in the folded string
    mask = picked(want, pick, 0, 0)
    assert mask.sum() > picked(fz.words(pats, ks, s.rows.strs), pick, 0, 0).sum() > 0      # more than the unfolded strings hold: 'PASSWORD ...'
    sel = s.res.select_device(bound, any=pick)
    check_sel(s, s.res, sel, mask)                                                           # the ORIGINAL strings
    sel.free(); bound.free(); lab.free(); fs.free(); fold.free()


# ---- what the selections and the order make of the words

def test_select_by_the_words(sources):
    s = sources("merged")
    pats, ks, nocase = fz.SETS["nine"]
    fs = s.sc.fuzzy_set(pats, ks)
    lab = s.res.fuzzy_device(fs)
    want = fz.words(pats, ks, s.rows.strs)
    for masks in (dict(any=1), dict(any=0x1FF), dict(all=1 | 1 << 5), dict(any=1 << 2 | 1 << 3, none=1), dict(none=0x1FF), dict(any=1 << 9)):
        mask = picked(want, masks.get("any", 0), masks.get("all", 0), masks.get("none", 0))
        assert 0 < mask.sum() < s.rows.n or masks in (dict(any=1 << 9), dict(all=1 | 1 << 5)), masks      # (a bit no pattern owns selects nothing)
        sel = s.res.select_device(lab, **masks)
        check_sel(s, s.res, sel, mask)
        sel.free()
    # ordered: the first ten of the findings that hold 'password' within two errors
    part = np.nonzero(picked(want, 1, 0, 0))[0]
    order = sorted(part.tolist(), key=lambda i: s.rows.strs[i])[:10]
    out = s.res.order_device(labels=lab, any=1, limit=10)
    check_records(s.sc, out, s.rows.take(np.array(order, dtype=np.int64)), True, "the ten first in order")
    assert out.order_info["findings"] == len(part) > 10 and out.order_info["kept"] == 10      # (findings: those the pick lets take part)
    out.free(); lab.free(); fs.free()


def test_no_errors_selects_what_the_substring_selection_selects(sources):
    s = sources("merged")
    pats, ks, _ = fz.SETS["exact"]
    fs = s.sc.fuzzy_set(pats, max_errors=0)
    lab = s.res.fuzzy_device(fs)
    mask = s.rows.mask(lambda x: pats[0] in x or pats[1] in x)
    assert 0 < mask.sum() < s.rows.n
    same(words_of(s.sc, lab, s.res) != 0, mask, "k = 0 against `in`")
    by_words = s.res.select_device(lab, any=3)
    check_sel(s, s.res, by_words, mask)
    by_substring = s.res.select_device(pats)
    check_sel(s, s.res, by_substring, mask)
    assert printed_on_device(s.sc, by_words) == printed_on_device(s.sc, by_substring) == s.rows.take(mask).text()
    by_words.free(); by_substring.free(); lab.free(); fs.free()


def test_refusals(sources):
    s, other, L = sources("merged"), sources("wave", 65), sx.lib()
    pats, ks, _ = fz.SETS["one"]
    fs = s.sc.fuzzy_set(pats, ks)
    out = C.c_void_p(0xDEAD0)
    assert L.sx_result_fuzzy_device(s.sc.h, s.res.h, None, 0, C.byref(out)) == sx.SX_E_INVALID and out.value is None
    assert L.sx_result_fuzzy_device(s.sc.h, s.res.h, fs.h, 0, None) == sx.SX_E_INVALID
    ls = s.sc.label_set([b"a"])
    with pytest.raises(sx.SxError) as e:
        s.res.fuzzy_device(ls)
    assert e.value.code == sx.SX_E_INVALID
    ls.free()
    # words of another result
    lab, theirs = s.res.fuzzy_device(fs), other.res.fuzzy_device(fs)
    for call in (lambda: s.res.select_device(theirs, any=1), lambda: other.res.order_device(labels=lab, any=1)):
        with pytest.raises(sx.SxError) as e:
            call()
        assert e.value.code == sx.SX_E_INVALID
    lab.free(); theirs.free()
    fs.reset()
    # a result in host memory, and one whose memory a later scan has reused: nothing is counted
    data = lp.buffer(fz.lines(65)) + b"\x80" * 8192
    plain = sx.Scanner(fp.ms1(), device=0)
    host = plain.scan(data, file_id=1)
    assert len(host) == 65
    out = C.c_void_p(0xDEAD0)
    assert L.sx_result_fuzzy_device(plain.h, host.h, fs.h, 0, C.byref(out)) == sx.SX_E_STATE and out.value is None
    assert b"host memory" in L.sx_last_error(plain.h)
    host.free(); plain.close()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SX_WAVE_REPLAY", "1")
        sc = sx.Scanner(fp.ms1(), device=0, result_on_device=True)
    old = sc.scan(data, file_id=1)
    old.fuzzy_device(fs).free()
    assert fs.read()[0] == [int(fz.words(pats, ks, fz.lines(65)).sum())]
    new = sc.scan(data, file_id=1)
    with pytest.raises(sx.SxError) as e:
        old.fuzzy_device(fs)
    assert e.value.code == sx.SX_E_STATE and "reused" in str(e.value)
    assert fs.read()[0] == [int(fz.words(pats, ks, fz.lines(65)).sum())]
    # a host-only context has no device for a set; the set outlives its context and counts for another
    new.free(); old.free(); sc.close()
    host_only = sx.Scanner(fp.ms1(), device=sx.SX_HOST_ONLY)
    with pytest.raises(sx.SxError) as e:
        host_only.fuzzy_set(pats, ks)
    assert e.value.code == sx.SX_E_STATE
    host_only.close()
    fs.reset()
    other.res.fuzzy_device(fs).free()
    assert fs.read()[0] == [int(fz.words(pats, ks, other.rows.strs).sum())]
    fs.free(); fs.free()
    with pytest.raises(sx.SxError):
        other.res.fuzzy_device(fs)
