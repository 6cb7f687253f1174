"""The kernels that work on a result lying in HBM (selection by substring, keyword set, regex and label; extraction; tally; labels;
distinct; the seen set) at the sizes at which their grid STRIDES: a workgroup is kRowsWaves wavefronts of 64 records, the grid is capped
at what the device holds at once (csrc/sx_rows_dev.hpp rows_grid), and only above

    R = CUs x kRowsGroupsPerCu x kRowsWaves x 64                                   records in ONE segment (the rows kernels)
    S = CUs x max(kDistinctGroupsPerCu, kSeenGroupsPerCu) x kRowsWaves x 64        (the distinct and seen kernels)

does a wavefront make a second trip through its loop: the stride step, the selections' extra wavefront at the head of a later trip, the
LDS counters and minima that accumulate across trips before one flush, the per-wavefront totals before one add, the `continue` in
front of seen_add_kernel's shuffles, distinct's rounds when a workgroup claims in two trips.  The constants are read from the
sources and the CU count from the device, so the sources below are as large as that takes:

    two_trips    MS2 on S + 97 lines: 2 S + 194 merged findings, packed, strings in one range; two full trips of every kernel, some
                 workgroups a third, the last wavefront partial
    exact        MS1 (the wave path) on prefix(R): R findings — one trip exactly, the selections' extra wavefront alone in trip 2
    one_over     MS1 on prefix(R + 1): trip 2 of the rows kernels holds one record, SENTINEL
    one_over_s   MS1 on prefix(S + 1): the same for the distinct and seen kernels

Every expected value comes from the oracle's text (tests/result_plant.py expected()) and plain Python or numpy over its strings; no
value comes from a product Scanner.  tests/test_gpu_result_edges.py runs the same operations at the wavefront-edge counts."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import result_plant as rp
import stringsext_amd as sx
from test_gpu_result_on_device_multi import F16, F32
from test_gpu_seen_device import entry_bytes
from test_gpu_select_device import info_tuple

pytestmark = pytest.mark.gpu

FIRST, REPEATED, SEEN, SHIFT = sx.SX_DISTINCT_FIRST, sx.SX_DISTINCT_REPEATED, sx.SX_DISTINCT_SEEN, sx.SX_DISTINCT_COUNT_SHIFT
CANNOT_OCCUR = b"\x02\x02"
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stringsext_amd", "csrc")
LDS_IDS = 4096          # the unique ids below it are counted in LDS (sx_seltally_build.hpp: kSeltallyLdsIds)


def constant(name):
    """`constexpr uint32_t name = N;` from the sources: a constant that is gone or spelt otherwise fails the tests, not their coverage"""
    found = set()
    for path in sorted(glob.glob(os.path.join(CSRC, "*.h*"))):
        with open(path) as f:
            found |= {int(v) for v in re.findall(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)u?\s*;" % name, f.read())}
    assert len(found) == 1, (name, found)
    return found.pop()


def trip_sizes():
    """(R, S): the records of one segment that fill one trip of the rows kernels, and of the distinct and seen kernels"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count      # hipDeviceAttributeMultiprocessorCount: what rows_grid asks
    waves, recs = constant("kRowsWaves"), constant("kSelectRecs")
    assert cus > 0 and recs == 64
    return (cus * constant("kRowsGroupsPerCu") * waves * recs,
            cus * max(constant("kDistinctGroupsPerCu"), constant("kSeenGroupsPerCu")) * waves * recs)


def same(got, want, what, strs=None):
    """two arrays, with the first place at which they differ"""
    assert len(got) == len(want), (what, len(got), len(want))
    if not np.array_equal(got, want):
        i = int(np.nonzero(np.asarray(got) != np.asarray(want))[0][0])
        raise AssertionError("%s: %d records, first difference at %d: got %r, want %r%s"
                             % (what, len(want), i, got[i], want[i], "" if strs is None else " (%r)" % strs[i]))


def gathered(arena, off, ln):
    """the bytes of the strings [off, off + ln) of an arena, back to back"""
    out, step = [], 1 << 17
    for i0 in range(0, len(off), step):
        o, n = off[i0:i0 + step], ln[i0:i0 + step]
        out.append(arena[np.repeat(o - (np.cumsum(n) - n), n) + np.arange(int(n.sum()))])
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint8)


def check_records(sc, res, rows, back_to_back, what):
    """every segment of `res` downloaded: position, precision, completes, Mission, str_len and the strings' bytes against the oracle's
    rows; back_to_back: the layout rule of merged and selected segments"""
    segs = res.device_segments()
    assert len(res) == rows.n == sum(s[1] for s in segs), (what, len(res), rows.n)
    at = 0
    for fp, n, ap, alen, packed, info in segs:
        assert fp and ap and n > 0, what
        recs = np.frombuffer(sc.download(fp, n * (16 if packed else 32)), dtype=F16 if packed else F32)
        arena = np.frombuffer(sc.download(ap, alen), dtype=np.uint8)
        sl = slice(at, at + n)
        same(recs["position"], rows.position[sl], what + ": position")
        if packed:
            same(recs["flags"] & 3, rows.precision[sl], what + ": precision")
            same(recs["flags"] & 4 != 0, rows.completes[sl], what + ": completes")
            assert not np.any(recs["flags"] & 0xF8)
        else:
            same(recs["precision"], rows.precision[sl], what + ": precision")
            same(recs["completes"] != 0, rows.completes[sl], what + ": completes")
        same(recs["mission_id"], rows.mission[sl], what + ": mission_id")
        same(recs["str_len"].astype(np.uint64), rows.length[sl], what + ": str_len", rows.strs[sl])
        off, ln = recs["str_off"].astype(np.int64), recs["str_len"].astype(np.int64)
        if back_to_back:
            assert off[0] == 0 and np.array_equal(off[1:], (off + ln)[:-1]) and int(off[-1] + ln[-1]) == alen == int(ln.sum()), what
        else:
            assert int((off + ln).max()) <= alen, what
        want = np.frombuffer(b"".join(rows.strs[sl]), dtype=np.uint8)
        got = gathered(arena, off, ln)
        if not np.array_equal(got, want):
            i = int(np.searchsorted(np.cumsum(ln), int(np.nonzero(got != want)[0][0]), side="right"))
            raise AssertionError("%s: %d records, record %d: got %r, want %r" % (what, n, at + i, bytes(arena[off[i]:off[i] + ln[i]]), rows.strs[at + i]))
        at += n


def words_of(sc, lab, res):
    """a Labels object's words in print order as one uint64 array; an array per source segment, of the segment's size"""
    segs = lab.device_segments()
    assert [n for _, n in segs] == [s[1] for s in res.device_segments()] and all(p and p % 256 == 0 for p, _ in segs)
    return np.concatenate([np.frombuffer(sc.download(p, n * 8), dtype="<u8") for p, n in segs])


class Source:
    """a result on the device with the oracle's rows for it.  fresh() is the result to work on: the selections of a context use two
    blocks in turn, so a source that is itself a selection (tests/test_gpu_result_edges.py) is made again before every operation that
    selects from it"""

    def __init__(self, name, sc, res, rows, ms, back_to_back, remake=None):
        self.name, self.sc, self.res, self.rows, self.ms, self.back_to_back, self.remake = name, sc, res, rows, ms, back_to_back, remake
        self.sentinel_last = rows.strs[-1] == rp.SENTINEL       # (a prefix: the last record holds every pattern)
        self.cache = {}

    def fresh(self):
        if self.remake:
            self.res.free()
            self.res = self.remake()
        return self.res

    def memo(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    def close(self):
        self.res.free()


def scanned(name, ms, data, count, env=(), packed=True):
    """`data` scanned into a result that stays on the device, all of it in ONE segment of `count` records"""
    rows = rp.expected(ms, data)
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env:
            mp.setenv(k, v)
        sc = sx.Scanner(ms, device=0, result_on_device=True)          # (a context keeps the switches it was created under)
    res = sc.scan(data, file_id=1)
    segs = res.device_segments()
    assert len(res) == rows.n == count, (name, len(res), rows.n, count)
    assert max(s[1] for s in segs) == count and len(segs) == 1 and segs[0][0] and segs[0][4] == packed, [(s[0], s[1], s[4]) for s in segs]
    return Source(name, sc, res, rows, ms, back_to_back=len(ms) > 1)


@pytest.fixture(scope="module")
def sizes():
    r, s = trip_sizes()
    print("R = %d, S = %d" % (r, s))
    assert r > 0 and s >= r
    return r, s


@pytest.fixture(scope="module")
def two_trips(sizes):
    s = scanned("two_trips", rp.ms2(), rp.buffer(sizes[1] + 97), 2 * sizes[1] + 194)
    yield s
    s.close(); s.sc.close()


def one_mission(name, k):
    return scanned(name, rp.ms1(), rp.prefix(k), k, env=(("SX_WAVE_REPLAY", "1"),))


@pytest.fixture(scope="module")
def exact(sizes):
    s = one_mission("exact", sizes[0])
    yield s
    s.close(); s.sc.close()


@pytest.fixture(scope="module")
def one_over(sizes):
    s = one_mission("one_over", sizes[0] + 1)
    yield s
    s.close(); s.sc.close()


@pytest.fixture(scope="module")
def one_over_s(sizes):
    s = one_mission("one_over_s", sizes[1] + 1)
    yield s
    s.close(); s.sc.close()


ALL = ["two_trips", "exact", "one_over", "one_over_s"]
ROWS = ["two_trips", "exact", "one_over"]              # the sources that are about the rows kernels
HASHED = ["two_trips", "one_over_s"]                   # ... about the distinct and seen kernels


# ---- the operations: each takes a Source and compares the whole answer ----

_sets = {}


def shared_set(name, make):
    """a compiled set, made once: it owns its device memory and any context on the device may use it (include/stringsext_amd.h)"""
    if name not in _sets:
        _sets[name] = make()
    return _sets[name]


def check_selection(s, res, sel, mask, rows=None):
    """`sel`, selected from `res` whose rows are `rows`, against the rows the bool array `mask` keeps; returns them"""
    rows = rows or s.rows
    want = rows.take(mask)
    assert len(sel) == want.n, (s.name, len(sel), want.n)
    if want.n == 0:
        check_empty(sel)
        return want
    src, segs = res.device_segments(), sel.device_segments()
    assert len(src) == 1 and [(g[1], g[4], info_tuple(g[5])) for g in segs] == [(want.n, src[0][4], info_tuple(src[0][5]))]
    assert segs[0][0] % 256 == 0 and segs[0][2] == segs[0][0] + want.n * (16 if segs[0][4] else 32)     # [records][strings], 256-byte aligned
    check_records(s.sc, sel, want, True, "%s: selection of %d from %d" % (s.name, want.n, rows.n))
    return want


def check_empty(sel):
    """an empty result is in host memory, as every result without findings (include/stringsext_amd.h)"""
    assert len(sel) == 0 and sel.device_segments() == [] and sel.segments() == [] and sel.findings() == []
    for call in (lambda: sel.printed_device(radix="x"), lambda: sel.select_device(b"a")):
        with pytest.raises(sx.SxError) as e:
            call()
        assert e.value.code == sx.SX_E_STATE


def printed_on_device(sc, res):
    p, n = res.printed_device(n_inputs=1, radix="x")
    return rp.OUTPUT_BOM + sc.download(C.c_void_p(p), n) + b"\n"


def op_records(s):
    check_records(s.sc, s.fresh(), s.rows, s.back_to_back, s.name)


def op_printed(s):
    res = s.fresh()
    before = [(g[0], g[1], g[2], g[3]) for g in res.device_segments()]
    got, want = printed_on_device(s.sc, res), s.rows.text()
    assert len(got) == len(want) and got == want, (s.name, len(got), len(want))
    assert [(g[0], g[1], g[2], g[3]) for g in res.device_segments()] == before                           # printing moves nothing


SUBSTRING_CASES = ["one", "sixteen", "ignore_case", "invert"]


def op_select_substring(s, case):
    rows = s.rows
    folded = rp.NOCASE.lower()
    pats, flags, pred = {"one": (rp.SUBSTRING, {}, lambda x: rp.SUBSTRING in x),
                         "sixteen": (rp.SIXTEEN, {}, lambda x: any(p in x for p in rp.SIXTEEN)),
                         "ignore_case": (rp.NOCASE, dict(ignore_case=True), lambda x: folded in x.lower()),
                         "invert": (rp.SUBSTRING, dict(invert=True), lambda x: rp.SUBSTRING not in x)}[case]
    mask = rows.mask(pred)
    assert (not s.sentinel_last or mask[-1] != (case == "invert")) and (rows.n < 64 or 0 < mask.sum() < rows.n), (case, mask.sum())
    if case == "ignore_case" and rows.n > 1000:
        assert rows.mask(lambda x: folded in x).sum() < mask.sum()                                          # the fold decides something
    res = s.fresh()
    sel = res.select_device(pats, **flags)
    check_selection(s, res, sel, mask)
    if case == "invert":            # the plain selection and its inverse partition the source
        res = s.fresh()
        plain = res.select_device(pats)
        assert len(plain) + int(mask.sum()) == len(res) == rows.n
        plain.free()
    sel.free()


def op_select_all_and_none(s):
    """the empty complement: a selection that keeps every record, and one that keeps none"""
    res = s.fresh()
    everything = res.select_device(CANNOT_OCCUR, invert=True)
    check_selection(s, res, everything, np.ones(s.rows.n, dtype=bool))
    everything.free()
    res = s.fresh()
    nothing = res.select_device(CANNOT_OCCUR)
    check_empty(nothing)
    nothing.free()


def op_pattern_set(s):
    kw = rp.keyword_list()
    occ = s.memo("keyword occurrences", lambda: rp.occurrences(s.rows.uniq, kw))
    mask = rp.held_by_any(s.rows, occ)
    assert (mask[-1] or not s.sentinel_last) and (s.rows.n < 64 or 0 < mask.sum() < s.rows.n)
    ps = shared_set("keywords", lambda: s.sc.pattern_set(kw))
    assert ps.info()["n_patterns"] == len(kw)
    for invert in (False, True):
        res = s.fresh()
        sel = res.select_device(ps, invert=invert)
        check_selection(s, res, sel, mask != invert)
        sel.free()


def op_regex_set(s):
    rx = [rp.to_python(p) for p in rp.REGEXES]
    mask = s.rows.mask(lambda x: any(r.search(x) for r in rx))
    each = [s.rows.mask(r.search) for r in rx]
    assert (mask[-1] or not s.sentinel_last) and (s.rows.n < 512 or all(0 < m.sum() < mask.sum() for m in each))                   # every pattern decides something
    rs = shared_set("regexes", lambda: s.sc.regex_set(rp.REGEXES))
    for invert in (False, True):
        res = s.fresh()
        sel = res.select_device(rs, invert=invert)
        check_selection(s, res, sel, mask != invert)
        sel.free()


def op_extract(s):
    """grep -oE: per finding its matches in order, each the source's record with another string"""
    both = re.compile(b"|".join(rp.EXTRACTS))              # runs of one class and a literal: leftmost-first is leftmost-longest
    rows = s.rows
    per_class = [both.findall(u) for u in rows.uniq]
    count = np.array([len(m) for m in per_class], dtype=np.int64)[rows.inv]        # the matches per source record
    assert (count[-1] >= 2 or not s.sentinel_last) and count[0] >= 2 and (rows.n < 64 or (count == 0).any()) and all(m for ms in per_class for m in ms)
    index = np.repeat(np.arange(rows.n), count)
    want = rows.take(index, strs=[m for u in rows.inv.tolist() for m in per_class[u]])
    xs = shared_set("extracts", lambda: s.sc.extract_set(rp.EXTRACTS))
    res = s.fresh()
    ext = res.extract_device(xs)
    assert len(ext) == want.n == int(count.sum())
    segs = ext.device_segments()
    assert len(segs) == 1 and segs[0][1] == want.n and segs[0][4] == res.device_segments()[0][4]
    check_records(s.sc, ext, want, True, "%s: %d matches in %d records" % (s.name, want.n, rows.n))
    ext.free()


def op_tally(s):
    """hits per keyword (overlapping places count) and the first ordinal; a hot keyword among the ids that are counted in LDS and a hot
    one among those counted in HBM at once"""
    kw, rows, never = rp.tally_list(), s.rows, sx.SX_TALLY_NEVER
    occ = s.memo("tally occurrences", lambda: rp.occurrences(rows.uniq, kw))
    want = rp.tally_model(rows, occ, never, base=7)
    short, long_ = kw.index(rp.HOT_SHORT), kw.index(rp.HOT_LONG)
    assert want[0][short] >= rows.n // 2 and want[0][kw.index(b"777")] >= 3 and want[1][kw.index(b"c0ffee")] == 7
    if rows.n > 1000:
        assert want[0][long_] > rows.n // 100 and sum(1 for h in want[0] if h) > 30 and sum(1 for h in want[0] if not h) > 4000
    ts = shared_set("tally", lambda: s.sc.tally_set(kw))
    ts.reset()
    assert ts.info()["unique"] == len(kw) > LDS_IDS + 100
    assert ts.read() == ([0] * len(kw), [never] * len(kw))
    assert s.fresh().tally_device(ts, ordinal_base=7) == rows.n
    got = ts.read()
    assert got == want, (s.name, rows.n, [(p, g, w) for p, g, w in zip(kw, zip(*got), zip(*want)) if g != w][:8])
    d_hits, d_first, d_map, unique = ts.counters_device()
    ids = np.frombuffer(s.sc.download(d_map, 4 * len(kw)), dtype="<u4")
    assert ids[short] < LDS_IDS <= ids[long_]                                                           # which side counted what
    # the same result again, behind itself: the counters add up and the first ordinal stays
    s.res.tally_device(ts, ordinal_base=7 + rows.n)
    assert ts.read() == ([2 * h for h in want[0]], want[1])


def label_words(rows):
    rx = [rp.to_python(p) for p in rp.LABELS]
    return np.array([sum(1 << p for p, r in enumerate(rx) if r.search(u)) for u in rows.uniq], dtype=np.uint64)[rows.inv]


def picked(words, any_, all_, none):
    any_, all_, none = np.uint64(any_), np.uint64(all_), np.uint64(none)
    return ((words & any_) != 0 if any_ else np.ones(len(words), dtype=bool)) & ((words & all_) == all_) & ((words & none) == 0)


def op_label(s):
    rows, never, base = s.rows, sx.SX_LABEL_NEVER, 5
    want = s.memo("labels", lambda: label_words(rows))
    bits = [(want >> np.uint64(p)) & np.uint64(1) != 0 for p in range(len(rp.LABELS))]
    assert (want[-1] == (1 << len(rp.LABELS)) - 1 or not s.sentinel_last) and (rows.n < 512 or all(0 < b.sum() < rows.n for b in bits))
    ls = shared_set("labels", lambda: s.sc.label_set(rp.LABELS))
    ls.reset()
    assert ls.read() == ([0] * len(rp.LABELS), [never] * len(rp.LABELS))
    res = s.fresh()
    lab = res.label_device(ls, ordinal_base=base)
    same(words_of(s.sc, lab, res), want, s.name + ": labels", rows.strs)
    assert ls.read() == ([int(b.sum()) for b in bits], [base + int(np.argmax(b)) if b.any() else never for b in bits]), (s.name, rows.n)
    mask = picked(want, 0b000101, 0b001000, 0b010000)              # `-> ` or mmap, four digits in a row, not long
    assert rows.n < 512 or 0 < mask.sum() < rows.n
    sel = res.select_device(lab, any=0b000101, all=0b001000, none=0b010000)
    check_selection(s, res, sel, mask)
    sel.free(); lab.free()


def distinct_of(s, nocase):
    return s.memo(("distinct", nocase), lambda: rp.distinct_model(s.rows.strs, FIRST, REPEATED, SHIFT, nocase=nocase))


def op_distinct(s, nocase):
    rows = s.rows
    want, want_info, keys, _ = distinct_of(s, nocase)
    if rows.n > 1000:           # classes of three sizes at least (1, 2, 3 and more; twice that with two Missions), and a dominant one
        sizes = (want[want & np.uint64(FIRST) != 0] >> np.uint64(SHIFT)).astype(np.int64)
        assert len(np.unique(sizes)) >= 3 and sizes.min() == len(s.ms) and sizes.max() > rows.n // 100
    res = s.fresh()
    lab = res.distinct_device(ignore_case=nocase)
    same(words_of(s.sc, lab, res), want, "%s: distinct words%s" % (s.name, " under the fold" if nocase else ""), rows.strs)
    assert {k: lab.info[k] for k in ("findings", "distinct", "repeated")} == want_info, (s.name, lab.info, want_info)
    assert 1 <= lab.info["rounds"] <= want_info["distinct"] and lab.info["table_log2"] == next(p for p in range(1, 64) if 1 << p >= 2 * rows.n)
    sel = res.select_device(lab, any=FIRST)
    kept = check_selection(s, res, sel, want & np.uint64(FIRST) != 0)
    if not nocase:
        assert kept.strs == list(dict.fromkeys(rows.strs))                                              # sort -u in the original order
    else:
        assert [x.lower() for x in kept.strs] == keys
    sel.free(); lab.free()


class SeenModel:
    """tests/test_gpu_seen_device.py's Stream — a Python set carried from call to call — over a source's classes"""

    def __init__(self):
        self.held = set()

    def expect(self, distinct, add=True):
        """(the words, the counted fields of sx_seen_info) of one call over a source whose distinct_model() is `distinct`"""
        words, info, keys, inv = distinct
        was = np.array([k in self.held for k in keys], dtype=bool)
        new = [k for k, h in zip(keys, was.tolist()) if not h]
        info = dict(info, seen_findings=int(was[inv].sum()), seen_distinct=int(was.sum()), added_strings=len(new) if add else 0,
                    added_bytes=sum(entry_bytes(len(k)) for k in new) if add else 0)
        if add:
            self.held.update(new)
        return words | np.where(was[inv], np.uint64(SEEN), np.uint64(0)), info

    def held_info(self):
        return dict(strings=len(self.held), bytes=sum(entry_bytes(len(k)) for k in self.held))


COUNTED = ("findings", "distinct", "repeated", "seen_findings", "seen_distinct", "added_strings", "added_bytes")


def seen_call(s, ss, model, add=True):
    """one seen_device call against the model: the words, the info, what the set holds; returns the words"""
    want, want_info = model.expect(distinct_of(s, False), add)
    res = s.fresh()
    lab = res.seen_device(ss, add=add)
    try:
        same(words_of(s.sc, lab, res), want, "%s: seen words" % s.name, s.rows.strs)
        assert {k: lab.info[k] for k in COUNTED} == want_info, (s.name, lab.info, want_info)
        i = ss.info()
        assert dict(strings=i["strings"], bytes=i["bytes"]) == model.held_info(), (s.name, i, model.held_info())
    finally:
        lab.free()
    return want


def op_seen(s):
    """into an empty set sized exactly to what the source holds (100 % full afterwards, the table at a load of about 1/2); again into
    the full set; with add=False; a set one string too small"""
    full = SeenModel()
    full.expect(distinct_of(s, False))
    cap = full.held_info()
    ss, small, empty = s.sc.seen_set(cap["strings"], cap["bytes"]), s.sc.seen_set(max(1, cap["strings"] - 1), cap["bytes"]), s.sc.seen_set(cap["strings"], cap["bytes"])
    try:
        model = SeenModel()
        # add=False into an empty set: nothing seen, nothing added
        words = seen_call(s, empty, model, add=False)
        assert not (words & np.uint64(SEEN)).any() and empty.info()["strings"] == 0
        # every string is new: the set ends exactly full
        words = seen_call(s, ss, model)
        assert not (words & np.uint64(SEEN)).any()
        info = ss.info()
        assert (info["strings"], info["bytes"]) == (info["capacity_strings"], info["capacity_bytes"]) == (cap["strings"], cap["bytes"])
        assert info["table_log2"] == next(p for p in range(1, 64) if 1 << p >= 2 * cap["strings"])
        # again: every record SEEN, nothing added — with add and without
        for add in (True, False):
            words = seen_call(s, ss, model, add=add)
            assert (words & np.uint64(SEEN)).all() and ss.info() == info
        # one string too small: refused, and the set stays as it was
        if cap["strings"] > 1:
            before = small.info()
            out, sinfo = C.c_void_p(0xDEAD0), sx.SeenInfo()
            assert sx.lib().sx_result_seen_device(s.sc.h, s.fresh().h, small.h, 0, C.byref(out), C.byref(sinfo)) == sx.SX_E_NOMEM and out.value is None
            assert small.info() == before and before["strings"] == 0
            words = seen_call(s, small, SeenModel(), add=False)                                         # (a lookup is never refused)
            assert not (words & np.uint64(SEEN)).any()
    finally:
        ss.free(); small.free(); empty.free()


# ---- the tests: one per operation and source ----

def test_the_constants_are_read_from_the_sources(sizes):
    r, s = sizes
    assert constant("kRowsWaves") * constant("kSelectRecs") == 512 and r % 512 == 0 and s % 512 == 0
    with pytest.raises(AssertionError):
        constant("kNoSuchConstant")


@pytest.mark.parametrize("name", ALL)
def test_records_and_strings_as_they_lie(name, request):
    op_records(request.getfixturevalue(name))


@pytest.mark.parametrize("name", ALL)
def test_printed_device_is_the_oracles_text(name, request):
    op_printed(request.getfixturevalue(name))


@pytest.mark.parametrize("case", SUBSTRING_CASES)
@pytest.mark.parametrize("name", ROWS)
def test_select_by_substring(name, case, request):
    op_select_substring(request.getfixturevalue(name), case)


@pytest.mark.parametrize("name", ROWS)
def test_select_everything_and_nothing(name, request):
    op_select_all_and_none(request.getfixturevalue(name))


@pytest.mark.parametrize("name", ROWS)
def test_select_by_2000_keywords(name, request):
    op_pattern_set(request.getfixturevalue(name))


@pytest.mark.parametrize("name", ROWS)
def test_select_by_regex(name, request):
    op_regex_set(request.getfixturevalue(name))


@pytest.mark.parametrize("name", ROWS)
def test_extract(name, request):
    op_extract(request.getfixturevalue(name))


@pytest.mark.parametrize("name", ROWS)
def test_tally(name, request):
    op_tally(request.getfixturevalue(name))


@pytest.mark.parametrize("name", ROWS)
def test_labels(name, request):
    op_label(request.getfixturevalue(name))


@pytest.mark.parametrize("nocase", [False, True], ids=["plain", "ignore_case"])
@pytest.mark.parametrize("name", HASHED)
def test_distinct(name, nocase, request):
    op_distinct(request.getfixturevalue(name), nocase)


@pytest.mark.parametrize("name", HASHED)
def test_seen(name, request):
    op_seen(request.getfixturevalue(name))


def test_seen_into_a_set_that_another_context_filled(two_trips, exact):
    """the set holds the strings of `exact`'s source — another context on the same device, a prefix of two_trips' lines —: the
    intersection and the remainder, selected by the words"""
    model, both = SeenModel(), SeenModel()
    both.expect(distinct_of(exact, False)); both.expect(distinct_of(two_trips, False))
    cap = both.held_info()
    ss = exact.sc.seen_set(cap["strings"], cap["bytes"])
    try:
        seen_call(exact, ss, model)
        s = two_trips
        want, want_info = model.expect(distinct_of(s, False))
        was = want & np.uint64(SEEN) != 0
        assert was.any() and not was.all() and 0 < want_info["seen_distinct"] < want_info["distinct"] and want_info["added_strings"] > 0
        res = s.fresh()
        lab = res.seen_device(ss)
        same(words_of(s.sc, lab, res), want, "two_trips behind exact: seen words", s.rows.strs)
        assert {k: lab.info[k] for k in COUNTED} == want_info, (lab.info, want_info)
        info = ss.info()
        assert (info["strings"], info["bytes"]) == (cap["strings"], cap["bytes"]) == (info["capacity_strings"], info["capacity_bytes"])
        for masks, mask in ((dict(any=SEEN), was), (dict(none=SEEN), ~was)):
            sel = res.select_device(lab, **masks)
            check_selection(s, res, sel, mask)
            sel.free()
        lab.free()
    finally:
        ss.free()
