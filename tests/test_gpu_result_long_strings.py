"""Every operation on a result that lies in HBM — print, the selections by substring, keyword set, regex, label and label range,
extraction, tally, labels, distinct, the seen set with merge, grow, export / import, add_strings and counts, and the order — on LONG
strings: the lines of tests/long_plant.py, up to 1024 bytes under `-q 1024`, up to 256 bytes of multi-byte characters on the wave path,
and 16 000 and 64 000 bytes at `-q 16000`, the documented bound of packed merged records.  tests/result_plant.py's lines, which every
other GPU test of the family takes, end at 60 bytes.

The sources
    two      long_plant.msl2(): two Missions, merged, packed records, strings back to back
    parts    the same under SX_MERGE_PART_FINDINGS=1024: three parts or more, and classes with members in two of them
    one      long_plant.msl1(): one UTF-8 Mission at -q 255, the longest line the lane-per-region replay takes on the device: unpacked
             records, strings of up to 1000 bytes where the writer put them
    wave     long_plant.msw(): one UTF-8 Mission on the wave path at -q 64, packed records
    limit    long_plant.limit_ms(): two Missions at -q 16000

Every expected value is a model over the oracle's strings (result_plant.expected(): Python's `in`, `re`, sorted(), dict and Counter),
and every comparison is exact; no value comes from a product Scanner.  tests/test_long_plant.py asserts what the lines hold, and feeds
a prefix of them to the lane functions' CPU harnesses."""
import collections
import ctypes as C
import re
import time

import numpy as np
import pytest

import long_plant as lp
import result_plant as rp
import stringsext_amd as sx
import sxo_binding as sxo
from test_gpu_result_strides import (SeenModel, Source, check_empty, check_records, distinct_of, op_seen, picked, printed_on_device, same,
                                     seen_call, words_of)
from test_gpu_seen_device import entry_bytes
from test_order_core import fold, model

pytestmark = pytest.mark.gpu

FIRST, REPEATED, SEEN, SHIFT = sx.SX_DISTINCT_FIRST, sx.SX_DISTINCT_REPEATED, sx.SX_DISTINCT_SEEN, sx.SX_DISTINCT_COUNT_SHIFT
QUIET, TWO_WINDOWS = b"\x80", 2 * 4096      # a byte in which no Mission here reads a character; the wave path takes buffers of two windows or more
NAMES = ["two", "parts", "one", "wave"]
LONG = ("two", "parts")                     # the sources that hold every line of long_plant.lines()


def make(name):
    env, kw = (), {}
    if name in ("two", "parts"):
        ms, data = lp.msl2(), lp.buffer(lp.lines())
        env = (("SX_MERGE_PART_FINDINGS", "1024"), ("SX_MERGE_PART_MIB", "1")) if name == "parts" else ()
    elif name == "one":
        ms, data, env, kw = lp.msl1(), lp.buffer(lp.one_lines()), (("SX_WAVE_REPLAY", "0"),), dict(device_replay=True)
    elif name == "wave":
        ms, data, env = lp.msw(), lp.buffer(lp.wave_lines()), (("SX_WAVE_REPLAY", "1"),)
        data += QUIET * max(0, TWO_WINDOWS - len(data))
    else:
        ms, data = lp.limit_ms(), lp.buffer(lp.limit_lines())
    rows = rp.expected(ms, data)
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env:
            mp.setenv(k, v)
        sc = sx.Scanner(ms, device=0, result_on_device=True, **kw)      # (a context keeps the switches it was created under)
    res = sc.scan(data, file_id=1)
    segs = res.device_segments()
    assert len(res) == rows.n and all(g[0] for g in segs), (name, len(res), rows.n)
    # the kind of segments: the lane-per-region replay's records are sx_finding, every other source's are packed
    assert [g[4] for g in segs] == [name != "one"] * len(segs), (name, [g[4] for g in segs])
    if name == "parts":
        seg_of = [k for k, g in enumerate(segs) for _ in range(g[1])]
        first_seg = {}
        split = {s for k, s in zip(seg_of, rows.strs) if first_seg.setdefault(s, k) != k}
        assert len(segs) >= 3 and any(len(s) == 1024 for s in split), (len(segs), len(split))      # a deep family's class has members in two parts
    elif name != "one":
        assert len(segs) == 1, (name, len(segs))
    s = Source(name, sc, res, rows, ms, back_to_back=len(ms) > 1)
    s.data = data
    return s


@pytest.fixture(scope="module")
def sources():
    made = {}

    def get(name):
        if name not in made:
            made[name] = make(name)
        return made[name]
    yield get
    for s in made.values():
        s.close(); s.sc.close()


@pytest.fixture(params=NAMES)
def src(request, sources):
    return sources(request.param)


def check_sel(s, res, sel, mask, rows=None):
    """`sel`, selected from `res` whose rows are `rows`, against the rows the bool array `mask` keeps: a segment per source segment
    that has a selected record, of the source's record type, its strings back to back; returns the kept rows"""
    rows = rows or s.rows
    want = rows.take(mask)
    assert len(sel) == want.n, (s.name, len(sel), want.n)
    if want.n == 0:
        check_empty(sel)
        return want
    at, expect = 0, []
    for g in res.device_segments():
        k = int(mask[at:at + g[1]].sum())
        at += g[1]
        if k:
            expect.append((k, g[4]))
    assert [(g[1], g[4]) for g in sel.device_segments()] == expect, (s.name, expect)
    check_records(s.sc, sel, want, True, "%s: selection of %d from %d" % (s.name, want.n, rows.n))
    return want


# ---- the records as they lie, and print

def test_records_and_strings_as_they_lie(src):
    check_records(src.sc, src.res, src.rows, src.back_to_back, src.name)
    assert int(src.rows.length.max()) == {"two": 1024, "parts": 1024, "wave": 256, "one": 966 + 9}[src.name]


def test_printed_device_is_the_oracles_text(src):
    s = src
    got, want = printed_on_device(s.sc, s.res), s.rows.text()
    assert len(got) == len(want) and got == want, (s.name, len(got), len(want))
    bare = sxo.run_cli(s.ms, [s.data], radix="x", no_metadata=True)
    p, n = s.res.printed_device(n_inputs=1, radix="x", no_metadata=True)
    assert rp.OUTPUT_BOM + s.sc.download(C.c_void_p(p), n) + b"\n" == bare, s.name


# ---- the selections

SIXTEEN = [lp.NEEDLE, lp.NEEDLE64, b"tail3", b"77777", b"{needle", b"needle}", b"no such", b"uid=10:835", b"\xd0\xb6\xd0\xb6 ", b"(nee", b"TAIL1", b"0000 ",
           b"#", b"99999999", "語".encode(), b"zz"]
SUBSTRING_CASES = ["needle", "longest", "split halves", "ignore_case", "invert", "sixteen"]


@pytest.mark.parametrize("case", SUBSTRING_CASES)
def test_select_by_substring(src, case):
    s, rows = src, src.rows
    h = len(lp.NEEDLE) // 2
    up = [lp.NEEDLE.upper(), b"TAIL1"]
    pats, flags, pred = {"needle": (lp.NEEDLE, {}, lambda x: lp.NEEDLE in x),
                         "longest": (lp.NEEDLE64, {}, lambda x: lp.NEEDLE64 in x),
                         "split halves": ([lp.NEEDLE[:h], lp.NEEDLE[h:]], {}, lambda x: lp.NEEDLE[:h] in x or lp.NEEDLE[h:] in x),
                         "ignore_case": (up, dict(ignore_case=True), lambda x: any(p.lower() in x.lower() for p in up)),
                         "invert": (lp.NEEDLE, dict(invert=True), lambda x: lp.NEEDLE not in x),
                         "sixteen": (SIXTEEN, {}, lambda x: any(p in x for p in SIXTEEN))}[case]
    mask = rows.mask(pred)
    if case == "needle":
        # at offset 0, deep in a long line, as a line's last bytes — and the pair that holds it split is not selected
        held = [x for x in rows.uniq if lp.NEEDLE in x]
        assert any(x.startswith(lp.NEEDLE) for x in held) and any(x.endswith(lp.NEEDLE) and len(x) > 200 for x in held)
        pairs = [i for i in range(rows.n - 1) if rows.strs[i].endswith(lp.NEEDLE[:h]) and rows.strs[i + 1].startswith(lp.NEEDLE[h:])]
        assert pairs and not mask[pairs].any() and not mask[np.array(pairs) + 1].any()
    if case == "split halves":
        assert mask.sum() > rows.mask(lambda x: lp.NEEDLE in x).sum()             # the halves are found where the whole is not
    if case == "ignore_case" and s.name != "wave":      # (every other source has upper-case copies)
        assert mask.sum() > rows.mask(lambda x: any(p.lower() in x for p in up)).sum() > 0             # the fold decides something
    if case in ("needle", "sixteen", "invert"):
        assert 0 < mask.sum() < rows.n
    sel = s.res.select_device(pats, **flags)
    check_sel(s, s.res, sel, mask)
    sel.free()


def test_select_by_a_keyword_set_with_a_keyword_of_255_bytes(src):
    s, rows = src, src.rows
    kw = rp.keyword_list()[:300] + [lp.KEYWORD255, lp.NEEDLE, b"7" * 255, b"tail3", b"(nee"] + rp.keyword_list()[300:600]
    occ = s.memo("keyword occurrences", lambda: rp.occurrences(rows.uniq, kw))
    mask = rp.held_by_any(rows, occ)
    assert 0 < mask.sum() < rows.n and (s.name not in LONG or (occ[300] and occ[302]))
    h = len(lp.KEYWORD255) // 2
    pairs = [i for i in range(rows.n - 1) if rows.strs[i].endswith(lp.KEYWORD255[:h]) and rows.strs[i + 1].startswith(lp.KEYWORD255[h:])]
    assert s.name not in LONG or (pairs and not mask[pairs].any())                   # the keyword split between two findings is no hit
    ps = s.sc.pattern_set(kw)
    try:
        for invert in (False, True):
            sel = s.res.select_device(ps, invert=invert)
            check_sel(s, s.res, sel, mask != invert)
            sel.free()
    finally:
        ps.free()


def test_select_by_regex(src):
    s, rows = src, src.rows
    rx = [rp.to_python(p) for p in lp.REGEXES]
    mask = rows.mask(lambda x: any(r.search(x) for r in rx))
    if s.name in LONG:
        assert all(0 < rows.mask(r.search).sum() < rows.n for r in rx)
    rs = s.sc.regex_set(lp.REGEXES)
    try:
        for invert in (False, True):
            sel = s.res.select_device(rs, invert=invert)
            check_sel(s, s.res, sel, mask != invert)
            sel.free()
    finally:
        rs.free()


def test_select_by_labels_and_range_and_a_selection_of_a_selection(src):
    s, rows = src, src.rows
    words, _, _, _ = distinct_of(s, False)
    d = s.res.distinct_device()
    try:
        same(words_of(s.sc, d, s.res), words, s.name + ": distinct words", rows.strs)
        count = (words >> np.uint64(SHIFT)).astype(np.int64)
        lo = 5 if s.name in LONG else 3
        often = count >= lo
        assert 0 < often.sum() < rows.n
        sel = s.res.select_range_device(d, SHIFT, 32, lo, 1 << 31)
        kept = check_sel(s, s.res, sel, often)
        # a selection OF that selection: its strings lie back to back, whatever the source's did
        inner = kept.mask(lambda x: b"tail" in x or lp.NEEDLE in x or "語".encode() in x)
        again = sel.select_device([b"tail", lp.NEEDLE, "語".encode()])
        check_sel(s, sel, again, inner, rows=kept)
        again.free(); sel.free()
        firsts = s.res.select_device(d, any=FIRST, none=REPEATED)                  # uniq -u
        mask = picked(words, FIRST, 0, REPEATED)
        assert 0 < mask.sum() < rows.n or s.back_to_back
        check_sel(s, s.res, firsts, mask)
        firsts.free()
    finally:
        d.free()


# ---- extraction, tally, labels

def test_extract(src):
    s, rows = src, src.rows
    both = re.compile(b"|".join(lp.EXTRACTS))              # runs of one class and a literal: leftmost-first is leftmost-longest
    per_class = [both.findall(u) for u in rows.uniq]
    count = np.array([len(m) for m in per_class], dtype=np.int64)[rows.inv]
    want = rows.take(np.repeat(np.arange(rows.n), count), strs=[m for u in rows.inv.tolist() for m in per_class[u]])
    if s.name in LONG:
        assert count.max() == 100 and want.n > rows.n and lp.ONE_MATCH in want.strs and (count == 0).any()      # more matches than findings
    xs = s.sc.extract_set(lp.EXTRACTS)
    try:
        ext = s.res.extract_device(xs)
        assert len(ext) == want.n == int(count.sum())
        check_records(s.sc, ext, want, True, "%s: %d matches in %d records" % (s.name, want.n, rows.n))
        if s.name in LONG:
            dense = rows.strs.index(lp.DENSE)
            at = int(count[:dense].sum())
            assert want.strs[at:at + 100] == lp.DENSE.split(b" ") and len(set(want.position[at:at + 100].tolist())) == 1      # the finding's record, a hundred times
        ext.free()
    finally:
        xs.free()


def test_tally(src):
    s, rows, never = src, src.rows, sx.SX_TALLY_NEVER
    kw = lp.TALLY
    occ = rp.occurrences(rows.uniq, kw)
    want = rp.tally_model(rows, occ, never, base=7)
    if s.name == "one":
        assert want[0][0] >= 239 and want[0][1] >= 238
    if s.name in LONG:
        mult = len(s.ms)
        assert want[0][0] >= 599 * mult and want[0][1] >= 598 * mult and want[0][2] == (600 - 254) * mult and want[0][4] > 0      # the overlapping run
    assert want[0][kw.index(b"no such keyword")] == 0 and want[0][kw.index(lp.NEEDLE)] > 0
    ts = s.sc.tally_set(kw)
    try:
        assert s.res.tally_device(ts, ordinal_base=7) == rows.n
        got = ts.read()
        assert got == want, (s.name, [(p[:20], g, w) for p, g, w in zip(kw, zip(*got), zip(*want)) if g != w])
    finally:
        ts.free()


def test_labels(src):
    s, rows, never, base = src, src.rows, sx.SX_LABEL_NEVER, 5
    rx = [rp.to_python(p) for p in lp.LABELS]
    want = np.array([sum(1 << p for p, r in enumerate(rx) if r.search(u)) for u in rows.uniq], dtype=np.uint64)[rows.inv]
    bits = [(want >> np.uint64(p)) & np.uint64(1) != 0 for p in range(len(lp.LABELS))]
    assert s.name not in LONG or all(0 < b.sum() < rows.n for b in bits)
    ls = s.sc.label_set(lp.LABELS)
    try:
        lab = s.res.label_device(ls, ordinal_base=base)
        same(words_of(s.sc, lab, s.res), want, s.name + ": labels", rows.strs)
        assert ls.read() == ([int(b.sum()) for b in bits], [base + int(np.argmax(b)) if b.any() else never for b in bits]), s.name
        mask = picked(want, 0b000101, 0b010000, 0b000010)             # `^fam` or the needle, 200 bytes or more, no digit at the end
        sel = s.res.select_device(lab, any=0b000101, all=0b010000, none=0b000010)
        check_sel(s, s.res, sel, mask)
        sel.free(); lab.free()
    finally:
        ls.free()


# ---- distinct and the seen set

@pytest.mark.parametrize("nocase", [False, True], ids=["plain", "ignore_case"])
def test_distinct(src, nocase):
    s, rows = src, src.rows
    want, want_info, keys, inv = distinct_of(s, nocase)
    if s.name in LONG:
        # lines of 1024 bytes that differ in their last byte alone fall into different classes, the copies into one
        a = next(x for x in rows.uniq if len(x) == 1024 and x[:-1] + b"#" in rows.uniq)
        assert rows.strs.count(a) >= 3 and (fold(a) if nocase else a) in keys and (fold(a[:-1] + b"#") if nocase else a[:-1] + b"#") in keys
        assert nocase == (want_info["distinct"] < distinct_of(s, False)[1]["distinct"])
    lab = s.res.distinct_device(ignore_case=nocase)
    try:
        same(words_of(s.sc, lab, s.res), want, "%s: distinct words%s" % (s.name, " under the fold" if nocase else ""), rows.strs)
        assert {k: lab.info[k] for k in ("findings", "distinct", "repeated")} == want_info, (s.name, lab.info, want_info)
        sel = s.res.select_device(lab, any=FIRST)
        kept = check_sel(s, s.res, sel, want & np.uint64(FIRST) != 0)
        assert [fold(x) if nocase else x for x in kept.strs] == [fold(k) if nocase else k for k in keys]
        sel.free()
    finally:
        lab.free()


def test_seen_into_an_empty_an_exact_and_a_too_small_set(src):
    op_seen(src)


def capacity(strs):
    keys = set(strs)
    return len(keys), sum(entry_bytes(len(k)) for k in keys)


def test_seen_strings_merge_grow_export_and_import(src):
    s, rows = src, src.rows
    n, nbytes = capacity(rows.strs)
    long_ones = sorted({x for x in rows.uniq if len(x) >= 200}, key=lambda x: (len(x), x))[-40:]
    extra = [b"not in the source " + x[18:] for x in long_ones[:5]] + [long_ones[-1][:-1] + b"~"]      # as long, and different in the last byte
    assert not set(extra) & set(rows.uniq) and max(entry_bytes(len(x)) for x in rows.uniq) > 72
    ss, other, empty = s.sc.seen_set(n, nbytes), s.sc.seen_set(n + 6, nbytes + sum(entry_bytes(len(x)) for x in extra)), s.sc.seen_set(n, nbytes)
    loaded = None
    try:
        s.res.seen_device(ss).free()
        assert sorted(ss.strings()) == sorted(set(rows.strs))
        # add_strings / contains with the long lines
        info = other.add_strings(extra + long_ones[:10] + extra)
        assert (info["source_strings"], info["already_held"], info["added_strings"]) == (len(extra) + 10, 0, len(extra) + 10)
        assert info["added_bytes"] == sum(entry_bytes(len(x)) for x in extra + long_ones[:10])
        assert other.contains(long_ones + extra) == [x in long_ones[:10] for x in long_ones] + [True] * len(extra)
        assert ss.contains(long_ones + extra) == [True] * len(long_ones) + [False] * len(extra)
        # merge into an empty set, into a set that holds a part, and into the full one
        info = empty.merge(ss)
        assert (info["source_strings"], info["already_held"], info["added_strings"], info["added_bytes"]) == (n, 0, n, nbytes)
        assert sorted(empty.strings()) == sorted(set(rows.strs))
        info = empty.merge(ss)
        assert (info["source_strings"], info["already_held"], info["added_strings"], info["added_bytes"]) == (n, n, 0, 0)
        info = other.merge(ss)
        assert (info["source_strings"], info["already_held"], info["added_strings"]) == (n, 10, n - 10)
        assert sorted(other.strings()) == sorted(set(rows.strs) | set(extra))
        held = other.info()
        assert (held["strings"], held["bytes"]) == (held["capacity_strings"], held["capacity_bytes"]) == (n + 6, nbytes + sum(entry_bytes(len(x)) for x in extra))
        # one string too many: refused, and the set is as it was; grown, it takes it
        one_more = [long_ones[-1][:-1] + b"%"]
        with pytest.raises(sx.SxError) as e:
            other.add_strings(one_more)
        assert e.value.code == sx.SX_E_NOMEM and other.info() == held
        other.grow(n + 7, held["bytes"] + entry_bytes(len(one_more[0])))
        assert other.add_strings(one_more)["added_strings"] == 1 and sorted(other.strings()) == sorted(set(rows.strs) | set(extra) | set(one_more))
        # export -> import: the same strings in the same entries, and the result is SEEN all over
        blob = other.export()
        loaded = s.sc.seen_set_from(blob)
        assert sorted(loaded.strings()) == sorted(other.strings()) and len(blob) > held["bytes"]
        lab = s.res.seen_device(loaded, add=False)
        assert (words_of(s.sc, lab, s.res) & np.uint64(SEEN) != 0).all() and lab.info["seen_distinct"] == n
        lab.free()
    finally:
        for x in (ss, other, empty, loaded):
            if x is not None:
                x.free()


def test_a_counted_set(src):
    s, rows = src, src.rows
    n, nbytes = capacity(rows.strs)
    pred = (lambda x: b"tail" in x or lp.NEEDLE in x)
    mask = rows.mask(pred)
    sub = [x for x, m in zip(rows.strs, mask.tolist()) if m]
    assert 0 < len(sub) < rows.n
    ss = s.sc.seen_set(n, nbytes, counted=True)
    try:
        s.res.seen_device(ss).free()
        sel = s.res.select_device([b"tail", lp.NEEDLE])
        assert len(sel) == len(sub)
        sel.seen_device(ss).free()
        sel.free()
        once, again = collections.Counter(rows.strs), collections.Counter(sub)
        assert ss.counts() == {x: (1 + (x in again), once[x] + again[x]) for x in once}
        want = np.array([(1 + (x in again)) << sx.SX_SEEN_RESULTS_SHIFT | (once[x] + again[x]) << sx.SX_SEEN_FINDINGS_SHIFT for x in rows.strs], dtype=np.uint64)
        lab = s.res.seen_counts_device(ss)
        same(words_of(s.sc, lab, s.res), want, s.name + ": count words", rows.strs)
        lab.free()
    finally:
        ss.free()


# ---- the order

def check_order(s, res, rows, key="string", labels=None, words=None, descending=False, any_=0, limit=0, shift=0, bits=64):
    """one call against the model (tests/test_order_core.py model()); returns the ordered result and its rows"""
    part = np.array([i for i in range(rows.n) if not any_ or int(words[i]) & any_], dtype=np.int64)
    if key in ("string", "nocase"):
        keys, kw = [fold(rows.strs[i]) if key == "nocase" else rows.strs[i] for i in part.tolist()], dict(by="string", ignore_case=key == "nocase")
    else:
        keys, kw = [int(words[i]) >> shift & (1 << bits) - 1 for i in part.tolist()], dict(by="field", shift=shift, bits=bits)
    order, info = model(keys, descending, limit, key in ("string", "nocase"))
    out = res.order_device(labels=labels if (any_ or key == "field") else None, descending=descending, any=any_, limit=limit, **kw)
    what = "%s: order by %s%s, any=%d, limit=%d, shift=%d, bits=%d" % (s.name, key, " descending" if descending else "", any_, limit, shift, bits)
    assert out.order_info == info, (what, out.order_info, info)
    want = rows.take(part[np.array(order[:info["kept"]], dtype=np.int64)])
    assert [(g[1], g[4]) for g in out.device_segments()] == [(want.n, False)], what      # one segment of unpacked records
    check_records(s.sc, out, want, True, what)
    return out, want


def test_order_by_string(src):
    s, rows = src, src.rows
    words, _, _, _ = distinct_of(s, False)
    d = s.res.distinct_device()
    try:
        out, want = check_order(s, s.res, rows)
        assert out.order_info["rounds"] == {"two": 129, "parts": 129, "wave": 33, "one": 975 // 8 + 1}[s.name]      # equal strings of 1024 bytes part in round 129
        # the limit falls inside a class of equal long strings: its first members, in print order
        cut = next(p for p in range(want.n - 1, 0, -1) if want.strs[p] == want.strs[p - 1] and len(want.strs[p]) >= 200)
        # order the ORDER again: the identity; and select from it
        again, _ = check_order(s, out, want)
        again.free(); out.free()
        out, want = check_order(s, s.res, rows)               # (the results of a context take two blocks in turn: a third call would write `out`'s)
        sel = out.select_device(lp.NEEDLE)
        check_sel(s, out, sel, want.mask(lambda x: lp.NEEDLE in x), rows=want)
        sel.free(); out.free()
        check_order(s, s.res, rows, limit=cut)[0].free()
        check_order(s, s.res, rows, descending=True)[0].free()
        check_order(s, s.res, rows, key="nocase")[0].free()
        check_order(s, s.res, rows, key="nocase", descending=True, limit=cut)[0].free()
        out, want = check_order(s, s.res, rows, labels=d, words=words, any_=FIRST)      # sort -u
        assert want.strs == sorted(set(rows.strs)) and out.order_info["tied"] == 0
        out.free()
    finally:
        d.free()


def test_order_by_a_field_of_1_32_33_and_64_bits(src):
    s, rows = src, src.rows
    words, _, _, _ = distinct_of(s, False)
    d = s.res.distinct_device()
    try:
        for shift, bits in ((SHIFT, 32), (1, 1), (SHIFT - 1, 33), (0, 64), (SHIFT, 2)):
            for descending in (False, True):
                out, want = check_order(s, s.res, rows, key="field", labels=d, words=words, descending=descending, shift=shift, bits=bits)
                assert out.order_info["rounds"] == 0
                out.free()
        out, want = check_order(s, s.res, rows, key="field", labels=d, words=words, descending=True, any_=FIRST, limit=20, shift=SHIFT, bits=32)      # uniq -c | sort -rn | head -20
        assert want.n == 20
        out.free()
    finally:
        d.free()


# ---- the documented bound: -q 16000

@pytest.fixture(scope="module")
def limit(sources):
    return sources("limit")


def test_the_limit_source_as_it_lies_and_printed(limit):
    s = limit
    assert int(s.rows.length.max()) == 64000 and sorted(set(s.rows.length.tolist()))[-2:] == [16000, 64000]
    check_records(s.sc, s.res, s.rows, True, s.name)
    got, want = printed_on_device(s.sc, s.res), s.rows.text()
    assert len(got) == len(want) and got == want, (len(got), len(want))


def test_the_limit_source_selected_by_the_last_bytes_of_64000(limit):
    s, rows = limit, limit.rows
    mask = rows.mask(lambda x: lp.LIMIT_NEEDLE in x)
    assert mask.sum() == 2 and rows.strs[int(np.argmax(mask))].endswith(lp.LIMIT_NEEDLE) and rows.length[int(np.argmax(mask))] == 64000
    for pats, m in ((lp.LIMIT_NEEDLE, mask), (b"#", rows.mask(lambda x: b"#" in x)), (lp.LIMIT_NEEDLE[1:] + b"\n", np.zeros(rows.n, dtype=bool))):
        sel = s.res.select_device(pats)
        check_sel(s, s.res, sel, m)
        sel.free()
    sel = s.res.select_device(lp.LIMIT_NEEDLE, invert=True)
    check_sel(s, s.res, sel, ~mask)
    sel.free()


def test_the_limit_source_distinct_and_seen(limit):
    s, rows = limit, limit.rows
    want, want_info, keys, _ = distinct_of(s, False)
    assert want_info["distinct"] < rows.n and len({k[:15999] for k in keys if len(k) == 16000}) == 1 < len({k for k in keys if len(k) == 16000})
    lab = s.res.distinct_device()
    same(words_of(s.sc, lab, s.res), want, "limit: distinct words", rows.strs)
    assert {k: lab.info[k] for k in ("findings", "distinct", "repeated")} == want_info
    lab.free()
    n, nbytes = capacity(rows.strs)
    ss = s.sc.seen_set(n, nbytes)
    try:
        model_ = SeenModel()
        seen_call(s, ss, model_)
        assert sorted(ss.strings()) == sorted(set(rows.strs)) and ss.info()["bytes"] == nbytes
        words = seen_call(s, ss, model_)
        assert (words & np.uint64(SEEN)).all()
    finally:
        ss.free()


def test_the_limit_source_in_order(limit):
    """by string over the whole source: the two copies of the line of 64 000 bytes part in round 8001 (about one second on an MI355X,
    the model's check included: the whole order stays, no `any=FIRST` is needed to keep it short)"""
    s, rows = limit, limit.rows
    t0 = time.perf_counter()
    out, want = check_order(s, s.res, rows)
    print("limit: %d rounds, order and check in %.2f s" % (out.order_info["rounds"], time.perf_counter() - t0))
    assert out.order_info["rounds"] == 64000 // 8 + 1 and out.order_info["tied"] >= 4
    out.free()
    words, _, _, _ = distinct_of(s, False)
    d = s.res.distinct_device()
    try:
        out, want = check_order(s, s.res, rows, labels=d, words=words, any_=FIRST, descending=True)
        assert want.strs == sorted(set(rows.strs), reverse=True)
        out.free()
    finally:
        d.free()
