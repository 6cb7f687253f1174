"""sx_result_distinct_device (include/stringsext_amd.h): which findings of a result that lies in HBM repeat an earlier finding's string,
one 64-bit word per finding, decided on the device (stringsext_amd/csrc/sx_distinct_dev.hip) by a tournament by hash, and what
sx_result_select_labels_device makes of the words: sort -u, the duplicates, uniq -d, uniq -u.  The expected value never comes from
the code under test: a second Scanner without the flag scans the same data and a Python dict over its findings' strings says which
are first, which are repeated and how often."""
import collections
import ctypes as C
import random
import re

import pytest

import refconfig as rc
import stringsext_amd as sx
from test_gpu_result_on_device_multi import case
from test_gpu_select_device import check_selection, downloaded, filtered, pointers
from test_gpu_select_set_device import Source, code_of
from test_host_logic import synth

pytestmark = pytest.mark.gpu

FIRST, REPEATED, SHIFT = sx.SX_DISTINCT_FIRST, sx.SX_DISTINCT_REPEATED, sx.SX_DISTINCT_COUNT_SHIFT


def strings(findings):
    return [f["s"].encode("utf-8") for f in findings]


def py_words(findings, nocase=False):
    """(the words in print order, info's first three fields) from a dict over the strings; bytes.lower() folds 'A'..'Z' and nothing else"""
    keys = [s.lower() if nocase else s for s in strings(findings)]
    size = collections.Counter(keys)
    seen, words = set(), []
    for k in keys:
        words.append((FIRST if k not in seen else 0) | (REPEATED if size[k] > 1 else 0) | min(size[k], 0xFFFFFFFF) << SHIFT)
        seen.add(k)
    return words, dict(findings=len(keys), distinct=len(size), repeated=sum(1 for c in size.values() if c > 1))


def decided(words, three=True):
    """duplicates and singletons, and a class of three or more (three=False: case "A", whose classes are an ASCII line's two findings): no
    comparison is empty"""
    firsts = [w for w in words if w & FIRST]
    assert 0 < len(firsts) < len(words) and any(w >> SHIFT >= (3 if three else 2) for w in firsts) and any(w >> SHIFT == 1 for w in firsts), \
        (len(firsts), len(words))


def flat(lab, src):
    """a Labels object's words in print order; an array per source segment, of the segment's size, as sx_result_label_device lays them out"""
    segs = lab.device_segments()
    assert [n for _, n in segs] == [s[1] for s in src] and all(p and p % 256 == 0 for p, _ in segs)
    return [w for seg in lab.download() for w in seg]


def counted(info):
    return {k: info[k] for k in ("findings", "distinct", "repeated")}


def check_words(s, nocase=False, all_f=None, res=None):
    """the words and the info of s.res (or `res`, whose findings are all_f) against the dict; returns (the Labels, the words)"""
    res, all_f = res or s.res, s.all_f if all_f is None else all_f
    src = res.device_segments()
    want, want_info = py_words(all_f, nocase)
    lab = res.distinct_device(ignore_case=nocase)
    got = flat(lab, src)
    assert got == want, next((i, hex(a), hex(b), all_f[i]["s"]) for i, (a, b) in enumerate(zip(got, want)) if a != b)
    assert counted(lab.info) == want_info, (lab.info, want_info)
    assert 1 <= lab.info["rounds"] <= want_info["distinct"] and pointers(res) == [(x[0], x[1], x[2], x[3], x[4]) for x in src]      # read, not moved
    return lab, want


@pytest.fixture(scope="module")
def case_a():
    """case "A" — four Missions, dense: the ascii and the utf-8 Mission find every ASCII line once each"""
    ms, data, _ = case("A")
    ref = sx.Scanner(ms, device=0)
    host = ref.scan(data, file_id=1)
    all_f = host.findings()
    host.free(); ref.close()
    assert len(all_f) > 1000
    return dict(ms=ms, data=data, all_f=all_f)


@pytest.mark.parametrize("name", ["A", "C", "D"])
def test_several_missions(name, case_a):
    """the merger's segments: sx_finding16 records, the strings of a segment in one range; "A": every ASCII line twice"""
    ms, data, _ = case(name)
    s = Source(ms, data, all_f=case_a["all_f"] if name == "A" else None)
    try:
        assert all(seg[4] for seg in s.src)
        lab, want = check_words(s)
        print(name, lab.info)
        if name != "D":          # ("D": one Mission's random lines of 40 characters or more — every string is the only one of its class)
            decided(want, three=name != "A")
        assert lab.info["table_log2"] == next(p for p in range(1, 64) if 1 << p >= 2 * len(want))
        lab.free()
    finally:
        s.close()


def test_the_four_selections_and_the_duplicates(case_a):
    s = Source(case_a["ms"], case_a["data"], all_f=case_a["all_f"])
    try:
        lab, want = check_words(s)
        decided(want, three=False)
        n, sizes = len(want), {}
        for name, (any_, all_, none) in (("sort -u", (FIRST, 0, 0)), ("dropped", (0, 0, FIRST)), ("uniq -d", (0, FIRST | REPEATED, 0)),
                                         ("uniq -u", (FIRST, 0, REPEATED))):
            kept = [f for f, w in zip(s.all_f, want) if (any_ == 0 or w & any_) and w & all_ == all_ and not w & none]
            assert 0 < len(kept) < n, (name, len(kept))
            sizes[name] = len(kept)
            sel = s.res.select_device(lab, any=any_, all=all_, none=none)
            check_selection(s.sc, s.src, sel, kept, s.all_f, s.ms, prints=False)
            sel.free()
        assert sizes["sort -u"] + sizes["dropped"] == n and sizes["uniq -d"] + sizes["uniq -u"] == sizes["sort -u"]
        assert sizes["sort -u"] == lab.info["distinct"] and sizes["uniq -d"] == lab.info["repeated"]
        # sort -u is what Python's dict keeps, in the original order
        assert [f["s"] for f, w in zip(s.all_f, want) if w & FIRST] == list(dict.fromkeys(f["s"] for f in s.all_f))
        lab.free()
    finally:
        s.close()


def test_one_mission_sparse_unpacked_segment():
    """the lane-per-region replay's segment: sx_finding records, strings where the writer put them; synth plants words of a short list"""
    data = synth(random.Random(78), 4_000_000, 1 / 400)
    s = Source(rc.missions(encodings=["utf-8"], chars_min="10"), data, device_replay=True)
    try:
        assert not any(seg[4] for seg in s.src)
        lab, want = check_words(s)
        decided(want)
        print("sparse", lab.info)
        sel = s.res.select_device(lab, any=FIRST)
        check_selection(s.sc, s.src, sel, [f for f, w in zip(s.all_f, want) if w & FIRST], s.all_f, s.ms, prints=False)
        sel.free(); lab.free()
    finally:
        s.close()


def test_classes_that_span_segments(case_a, monkeypatch):
    monkeypatch.setenv("SX_MERGE_PART_FINDINGS", "7000")
    monkeypatch.setenv("SX_MERGE_PART_MIB", "1")
    s = Source(case_a["ms"], case_a["data"], all_f=case_a["all_f"])
    try:
        assert len(s.src) >= 3
        seg_of = [k for k, seg in enumerate(s.src) for _ in range(seg[1])]
        first_seg, spans = {}, 0
        for k, x in zip(seg_of, strings(s.all_f)):
            spans += first_seg.setdefault(x, k) != k
        assert spans > 0                                  # a class whose first and a later member lie in different segments
        lab, want = check_words(s)
        decided(want, three=False)
        sel = s.res.select_device(lab, none=FIRST)
        check_selection(s.sc, s.src, sel, [f for f, w in zip(s.all_f, want) if not w & FIRST], s.all_f, s.ms, prints=False)
        sel.free(); lab.free()
    finally:
        s.close()


def small_input():
    """some 400 findings of two Missions: 200 lines of a pool of 60, each found by both, and a line that the two read differently"""
    rng = random.Random(33)
    pool = [bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz0123456789") for _ in range(rng.randrange(8, 30))) for _ in range(60)]
    lines = [rng.choice(pool) for _ in range(200)] + ["exactly one of these: \u00e4\u00f6\u00fc\u00df\u00e4\u00f6\u00fc\u00df".encode("utf-8")]
    return rc.missions(encodings=["ascii", "utf-8"], chars_min="5"), b"\n".join(lines) + b"\n" + bytes(4096)


def test_many_rounds_give_the_same_words(monkeypatch):
    ms, data = small_input()
    seen = {}
    for log2 in (None, 0, 3):
        if log2 is None:
            monkeypatch.delenv("SX_DISTINCT_TABLE_LOG2", raising=False)
        else:
            monkeypatch.setenv("SX_DISTINCT_TABLE_LOG2", str(log2))
        s = Source(ms, data, all_f=seen.get("all_f"))
        try:
            seen["all_f"] = s.all_f
            assert 200 <= len(s.all_f) <= 1000
            lab, want = check_words(s)
            decided(want)
            info = lab.info
            print(log2, info)
            assert seen.setdefault("words", want) == want
            if log2 is None:
                assert info["table_log2"] == next(p for p in range(1, 64) if 1 << p >= 2 * len(want))
            else:
                assert info["table_log2"] == log2
            if log2 == 0:
                assert info["rounds"] == info["distinct"] > 50
            if log2 == 3:
                assert info["distinct"] / 8 <= info["rounds"] <= info["distinct"]
            monkeypatch.delenv("SX_DISTINCT_TABLE_LOG2", raising=False)      # a context keeps the switch it was created under
            again = s.res.distinct_device()
            assert again.info == info
            again.free(); lab.free()
        finally:
            s.close()


def test_the_fold():
    ms, data, _ = case("D")
    lines = data.split(b"\n")
    long_ones = [ln for ln in lines[:400] if len(ln) >= 60]
    planted = [ln.upper() for ln in lines[5:400:7] if len(ln) >= 40] + [ln.lower() for ln in lines[8:400:14] if len(ln) >= 40] \
        + [ln.upper() for ln in long_ones[:3]] * 2                              # classes of three or more
    assert len(planted) > 50 and all(p.lower() != p or p.upper() != p for p in planted)
    data = data + b"\n" + b"\n".join(planted) + b"\n" + bytes(4096)
    s = Source(ms, data)
    try:
        folded, want_folded = check_words(s, nocase=True)
        plain, want_plain = check_words(s)
        decided(want_folded)
        assert folded.info["distinct"] < plain.info["distinct"] and want_folded != want_plain      # the fold joins classes the plain call keeps apart
        sel = s.res.select_device(folded, all=FIRST | REPEATED)
        assert len(sel) == folded.info["repeated"] > 30
        sel.free(); folded.free(); plain.free()
    finally:
        s.close()


def overlapping(s, p):
    return sum(1 for o in range(len(s) - len(p) + 1) if s.startswith(p, o))


def test_a_selection_an_extraction_and_what_follows_a_deduplication(case_a):
    s = Source(case_a["ms"], case_a["data"], all_f=case_a["all_f"])
    try:
        all_f, res, sc = s.all_f, s.res, s.sc
        # the distinct of a selection
        kept = filtered(all_f, b"ab")
        assert 0 < len(kept) < len(all_f)
        sel = res.select_device(b"ab")
        lab, want = check_words(s, all_f=kept, res=sel)
        decided(want, three=False)
        uniq = sel.select_device(lab, any=FIRST)
        assert downloaded(sc, uniq) == [f for f, w in zip(kept, want) if w & FIRST]
        uniq.free(); lab.free(); sel.free()
        # tally and print of the deduplicated result
        lab, want = check_words(s)
        uniq = res.select_device(lab, any=FIRST)
        first_f = [f for f, w in zip(all_f, want) if w & FIRST]
        words = [b"ab", b"00", b"E=", b"zz9"]
        ts = sc.tally_set(words)
        assert uniq.tally_device(ts) == len(first_f)
        hits = [sum(overlapping(x, p) for x in strings(first_f)) for p in words]
        assert ts.read()[0] == hits and hits[0] > 0 and hits[0] < sum(overlapping(x, b"ab") for x in strings(all_f))
        check_selection(sc, s.src, uniq, first_f, all_f, s.ms, prints=True)      # (last: the host accessors it ends with fetch the selection)
        ts.free(); uniq.free(); lab.free()
    finally:
        s.close()


def test_the_unique_matches_of_an_extraction_and_their_counts():
    ms, data, _ = case("D")
    s = Source(ms, data)
    try:
        matches = [dict(f, s=m.decode("utf-8")) for f in s.all_f for m in re.findall(rb"[a-z]{4,}", f["s"].encode("utf-8"))]
        xs = s.sc.extract_set([rb"[a-z]{4,}"])
        ext = s.res.extract_device(xs)
        assert len(ext) == len(matches) > 1000
        lab, want = check_words(s, all_f=matches, res=ext)
        decided(want)
        uniq = ext.select_device(lab, any=FIRST)
        got = [f["s"] for f in downloaded(s.sc, uniq)]
        counts = collections.Counter(m["s"] for m in matches)             # (a dict: in the order of the first occurrence)
        assert got == list(counts)
        assert [w >> SHIFT for w in want if w & FIRST] == list(counts.values())          # uniq -c: the high half of the words that have bit 0
        uniq.free(); lab.free(); ext.free(); xs.free()
    finally:
        s.close()


def test_two_calls_give_the_same_words_and_the_same_info(case_a):
    s = Source(case_a["ms"], case_a["data"], all_f=case_a["all_f"])
    try:
        one, two = s.res.distinct_device(), s.res.distinct_device()
        assert flat(one, s.src) == flat(two, s.src) and one.info == two.info and one.info["distinct"] > 0
        folded = [s.res.distinct_device(ignore_case=True) for _ in range(2)]
        assert flat(folded[0], s.src) == flat(folded[1], s.src) and folded[0].info == folded[1].info
        for x in [one, two] + folded:
            x.free()
    finally:
        s.close()


def raw_call(sc_h, res_h, flags, with_out=True, with_info=True):
    """the C entry point itself: (its code, *out afterwards — set to a sentinel before)"""
    out, info = C.c_void_p(0xDEAD0), sx.DistinctInfo()
    rc_ = sx.lib().sx_result_distinct_device(sc_h, res_h, flags, C.byref(out) if with_out else None, C.byref(info) if with_info else None)
    return rc_, out.value


def test_refusals_leave_no_labels_and_no_memory_behind(case_a):
    import torch
    a = case_a
    s = Source(a["ms"], a["data"], all_f=a["all_f"])
    sc, res = s.sc, s.res
    plain = sx.Scanner(a["ms"], device=0)
    host = plain.scan(a["data"], file_id=1)
    try:
        lab = res.distinct_device()
        leak = 8 * len(a["all_f"])                        # what one call that forgot its words would keep; its tables are five times that
        torch.cuda.mem_get_info(0)
        free_before = torch.cuda.mem_get_info(0)[0]                                       # (nothing but refused calls until it is read again)
        for _ in range(8):
            # bad flags; NULL arguments (info alone may be NULL); a result in host memory
            for flags in (sx.SX_SELECT_INVERT, 4, sx.SX_SELECT_ASCII_NOCASE | 2, 1 << 31):
                assert raw_call(sc.h, res.h, flags) == (sx.SX_E_INVALID, None)
            assert raw_call(None, res.h, 0) == (sx.SX_E_INVALID, None) and raw_call(sc.h, None, 0) == (sx.SX_E_INVALID, None)
            assert raw_call(sc.h, res.h, 0, with_out=False)[0] == sx.SX_E_INVALID
            assert raw_call(plain.h, host.h, 0) == (sx.SX_E_STATE, None)
            assert "host memory" in sx.lib().sx_last_error(plain.h).decode()
            assert code_of(host.distinct_device) == sx.SX_E_STATE
        assert torch.cuda.mem_get_info(0)[0] >= free_before - 4 * leak, (free_before, torch.cuda.mem_get_info(0)[0])
        rc_, out = raw_call(sc.h, res.h, 0, with_info=False)                          # (info may be NULL)
        assert rc_ == sx.SX_OK and out
        sx.lib().sx_labels_free(out)
        # labels of result X offered to result Y
        sel = res.select_device(lab, any=FIRST)
        assert code_of(lambda: sel.select_device(lab, any=FIRST)) == sx.SX_E_INVALID
        assert "not made from this result" in sx.lib().sx_last_error(sc.h).decode()
        sel.free()
        # a source whose block a later scan has reused
        res2 = sc.scan(a["data"], file_id=1)
        free_before = torch.cuda.mem_get_info(0)[0]
        for _ in range(8):
            assert raw_call(sc.h, res.h, 0) == (sx.SX_E_STATE, None)
        assert "reused" in sx.lib().sx_last_error(sc.h).decode()
        assert code_of(res.distinct_device) == sx.SX_E_STATE
        assert torch.cuda.mem_get_info(0)[0] >= free_before - 4 * leak, (free_before, torch.cuda.mem_get_info(0)[0])
        assert code_of(lambda: res2.select_device(lab, any=FIRST)) == sx.SX_E_INVALID     # the same place in HBM, another result
        res2.free()
        lab.free()
    finally:
        host.free(); plain.close(); res.free(); sc.close()
    # a closed Scanner
    assert code_of(res.distinct_device) == sx.SX_E_STATE
    # a host-only context has no device for it
    host_only = sx.Scanner(a["ms"], device=sx.SX_HOST_ONLY)
    empty = sx.Scanner(a["ms"], device=0, result_on_device=True)
    r = empty.scan(a["data"][:200_000], file_id=1)
    assert raw_call(host_only.h, r.h, 0) == (sx.SX_E_STATE, None)
    assert "host-only" in sx.lib().sx_last_error(host_only.h).decode()
    r.free(); empty.close(); host_only.close()
