"""sx_select_regex_create / sx_result_select_regex_device (include/stringsext_amd.h): the findings of a result that lies in HBM,
selected by compiled regular expressions on the device (stringsext_amd/csrc/sx_selre_dev.hip).  As in
tests/test_gpu_select_set_device.py the expected value never comes from the code under test: a second Scanner without the flag
scans the same data and Python's re.search filters its findings — every pattern rendered for Python with `$` as `\\Z`, folded sets
with re.IGNORECASE."""
import ctypes as C
import random
import re

import pytest

import refconfig as rc
import stringsext_amd as sx
from test_gpu_result_on_device_multi import case, download_segment
from test_gpu_select_device import check_selection, downloaded, filtered, pick_patterns, pointers, printed_by_python
from test_gpu_select_set_device import Source, code_of, filtered_many, keyword_list
from test_host_logic import synth
from test_selre_core import to_python
from test_wave_core import text_lines

pytestmark = pytest.mark.gpu


def re_filtered(findings, patterns, ignore_case=False, invert=False):
    patterns = [patterns] if isinstance(patterns, bytes) else patterns
    res = [re.compile(to_python(p), re.IGNORECASE if ignore_case else 0) for p in patterns]
    return [f for f in findings if any(r.search(f["s"].encode("utf-8")) for r in res) != invert]


@pytest.fixture(scope="module")
def case_a():
    """case "A" — four Missions, dense: packed records, one-range strings — with its findings"""
    ms, data, _ = case("A")
    ref = sx.Scanner(ms, device=0)
    host = ref.scan(data, file_id=1)
    all_f = host.findings()
    host.free(); ref.close()
    assert len(all_f) > 1000
    return dict(ms=ms, data=data, all_f=all_f)


SHAPES = [([rb"[0-9]{3}\.[0-9]"], False), ([rb"^[a-z]+:/"], False), ([rb"[A-H]{2}$"], False), ([rb"^.{0,30}$"], False),
          ([rb"(=|:)[a-z]*(=|:)"], False), ([rb"[a-h]{2}$", rb"^x[0-9]"], True)]


def test_several_missions_a_handful_of_patterns(case_a):
    a = case_a
    s = Source(a["ms"], a["data"], all_f=a["all_f"])
    try:
        assert all(seg[4] for seg in s.src)
        n = len(a["all_f"])
        for k, (pats, nocase) in enumerate(SHAPES):
            rs = s.sc.regex_set(pats, ignore_case=nocase)
            info = rs.info()
            assert info["n_patterns"] == len(pats) and info["nocase"] == int(nocase) and info["table_bytes"] == info["states"] * info["classes"] * 2
            assert info["lds_states"] == info["states"] and (info["end_states"] > 0) == any(p.endswith(b"$") for p in pats)
            want, rest = re_filtered(a["all_f"], pats, nocase), re_filtered(a["all_f"], pats, nocase, invert=True)
            print(f"{pats}{' folded' if nocase else ''}: {len(want)} of {n}; {info}")
            assert 0 < len(want) < n and len(want) + len(rest) == n           # the inputs cannot hide an empty comparison
            if nocase:
                assert len(want) > len(re_filtered(a["all_f"], pats))           # the fold decides something
            s.check(rs, want, prints=k == 0)
            s.check(rs, rest, invert=True)
            if nocase:
                with pytest.raises(ValueError):
                    s.res.select_device(rs, ignore_case=True)
            rs.free()
    finally:
        s.close()


def test_the_regex_the_set_and_the_list_agree_on_sixteen_literals(case_a):
    a = case_a
    s = Source(a["ms"], a["data"], all_f=a["all_f"])
    try:
        pats, _ = pick_patterns(a["all_f"])["sixteen"]
        rs, ps = s.sc.regex_set([re.escape(p) for p in pats]), s.sc.pattern_set(pats)
        assert rs.info()["states"] <= ps.info()["states"]                      # the same automaton, minimised
        want = filtered(a["all_f"], pats)
        assert 0 < len(want) < len(a["all_f"])
        for how in (rs, ps, pats):           # (one at a time: a selection is valid until the second one after it)
            sel = s.res.select_device(how)
            assert len(sel) == len(want) and downloaded(s.sc, sel) == want
            sel.free()
        rs.free(); ps.free()
    finally:
        s.close()


def test_anchors_at_the_edges_of_a_record(case_a):
    a = case_a
    s = Source(a["ms"], a["data"], all_f=a["all_f"])
    try:
        recs, arena = download_segment(s.sc, s.src[0])
        strs = [f["s"].encode("utf-8") for f in a["all_f"][:s.src[0][1]]]
        assert b"".join(strs) == arena                                             # back to back: neighbours in the list are neighbours in HBM
        everywhere = [f["s"].encode("utf-8") for f in a["all_f"]]
        pairs = []
        for i in range(0, len(strs) - 1, max(1, len(strs) // 200)):
            tail, head = strs[i][-3:], strs[i + 1][:3]
            if len(tail) == 3 and len(head) == 3 and not any(tail + head in x for x in everywhere):
                pairs.append((tail, head))
            if len(pairs) == 40:
                break
        assert len(pairs) >= 10 and all(t + h in arena for t, h in pairs)
        spans = s.sc.regex_set([re.escape(t + h) for t, h in pairs] + [re.escape(t) + b".?" + re.escape(h) for t, h in pairs[:20]])
        sel = s.res.select_device(spans)
        assert len(sel) == 0 and sel.device_segments() == []                       # as plain regexes they select nothing
        sel.free(); spans.free()
        tails = [re.escape(t) + b"$" for t, _ in pairs]
        want = [f for f in a["all_f"] if any(f["s"].encode("utf-8").endswith(t) for t, _ in pairs)]
        assert want == re_filtered(a["all_f"], tails) and len(pairs) <= len(want) < len(a["all_f"])
        rs = s.sc.regex_set(tails)
        s.check(rs, want)
        rs.free()
        heads = [b"^" + re.escape(h) for _, h in pairs]
        want = [f for f in a["all_f"] if any(f["s"].encode("utf-8").startswith(h) for _, h in pairs)]
        assert want == re_filtered(a["all_f"], heads) and len(pairs) <= len(want) < len(a["all_f"])
        rs = s.sc.regex_set(heads)
        s.check(rs, want)
        rs.free()
    finally:
        s.close()


def test_empty_matches(case_a):
    a = case_a
    s = Source(a["ms"], a["data"], all_f=a["all_f"])
    try:
        rs = s.sc.regex_set([b"a*"])
        assert rs.info()["states"] == 1
        everything = s.res.select_device(rs)
        check_selection(s.sc, s.src, everything, a["all_f"], a["all_f"], a["ms"], prints=False)
        none = s.res.select_device(rs, invert=True)
        assert len(none) == 0 and none.device_segments() == [] and none.segments() == [] and none.findings() == []
        assert code_of(lambda: none.select_device(rs)) == sx.SX_E_STATE             # an empty result is in host memory
        everything.free(); none.free(); rs.free()
    finally:
        s.close()


def test_a_table_larger_than_lds(case_a):
    a = case_a
    kw = keyword_list(a["all_f"], n=600)
    pats, cur = [], b""
    for k in kw:
        e = re.escape(k)
        if cur and len(cur) + 1 + len(e) > sx.SX_SELECT_REGEX_MAX_PATTERN_BYTES:
            pats.append(cur); cur = b""
        cur = cur + b"|" + e if cur else e
    pats.append(cur)
    assert len(pats) <= sx.SX_SELECT_REGEX_MAX_PATTERNS and all(len(p) <= 1024 for p in pats)
    want = filtered_many(a["all_f"], kw)
    assert 0 < len(want) < len(a["all_f"])
    ids, res = {id(f) for f in want}, [re.compile(p) for p in pats]
    for f in a["all_f"][::97]:
        assert any(r.search(f["s"].encode("utf-8")) for r in res) == (id(f) in ids)
    s = Source(a["ms"], a["data"], all_f=a["all_f"])
    try:
        rs, ps = s.sc.regex_set(pats), s.sc.pattern_set(kw)
        info = rs.info()
        print(len(kw), "keywords in", len(pats), "patterns:", info, "; as a pattern set:", ps.info())
        assert info["states"] > info["lds_states"] > 0 and info["states"] <= ps.info()["states"]
        s.check(rs, want)
        by_set = s.res.select_device(ps)
        assert downloaded(s.sc, by_set) == want
        by_set.free(); rs.free(); ps.free()
    finally:
        s.close()


def two_sets(findings):
    """an anchored and an unanchored set from the case's own strings: three heads and a tail; the middle of the median string, loosened"""
    strs = sorted({f["s"].encode("utf-8") for f in findings if len(f["s"].encode("utf-8")) >= 6})
    picks = [strs[k * len(strs) // 4] for k in range(1, 4)]
    anchored = [b"^(?:" + b"|".join(re.escape(p[:2]) for p in picks) + b")", re.escape(picks[0][-2:]) + b"$"]
    mid = strs[len(strs) // 2]
    at = (len(mid) - 5) // 2
    return anchored, [re.escape(mid[at:at + 2]) + b".{0,2}" + re.escape(mid[at + 4:at + 5]) + b"+"]


def two_patterns(s):
    n = len(s.all_f)
    for pats in two_sets(s.all_f):
        want = re_filtered(s.all_f, pats)
        print(f"{pats}: {len(want)} of {n}")
        assert 0 < len(want) < n
        rs = s.sc.regex_set(pats)
        s.check(rs, want)
        s.check(rs, re_filtered(s.all_f, pats, invert=True), invert=True)
        rs.free()


def test_unpacked_merger_records(monkeypatch, case_a):
    monkeypatch.setenv("SX_PACKED", "0")
    s = Source(case_a["ms"], case_a["data"], all_f=case_a["all_f"])
    try:
        assert all(not seg[4] for seg in s.src)
        two_patterns(s)
    finally:
        s.close()


def test_several_parts_are_several_segments(monkeypatch, case_a):
    monkeypatch.setenv("SX_MERGE_PART_FINDINGS", "7000")
    monkeypatch.setenv("SX_MERGE_PART_MIB", "1")
    s = Source(case_a["ms"], case_a["data"], all_f=case_a["all_f"])
    try:
        assert len(s.src) >= 3
        two_patterns(s)
        rs = s.sc.regex_set(two_sets(s.all_f)[1])
        sel = s.res.select_device(rs, invert=True)
        assert len(sel.device_segments()) >= 3
        sel.free(); rs.free()
    finally:
        s.close()


def test_one_mission_dense_packed_segment(monkeypatch):
    """the wave path's segment: sx_finding16 records, strings where the writer put them"""
    monkeypatch.setenv("SX_WAVE_REPLAY", "1")
    data = text_lines(random.Random(77), 3_000_000)
    s = Source(rc.missions(encodings=["ascii"], chars_min="4"), data)
    try:
        assert len(s.all_f) >= 100 and all(seg[4] for seg in s.src) and len(s.src) == 1
        two_patterns(s)
    finally:
        s.close()


def test_one_mission_sparse_unpacked_segment():
    """the lane-per-region replay's segment: sx_finding records"""
    data = synth(random.Random(78), 8_000_000, 1 / 400)
    s = Source(rc.missions(encodings=["utf-8"], chars_min="10"), data, device_replay=True)
    try:
        assert len(s.all_f) >= 100 and all(not seg[4] for seg in s.src)
        two_patterns(s)
    finally:
        s.close()


def test_composition_and_lifetime(case_a):
    a = case_a
    ms, data, all_f = a["ms"], a["data"], a["all_f"]
    s = Source(ms, data, all_f=all_f)
    sc, res, src = s.sc, s.res, s.src
    sets = pick_patterns(all_f)
    pa, pb = sets["one"][0], sets["three"][0]
    ra, rb_, rc_ = rb"[0-9]{2}", rb"^[a-z]", rb"[A-H]$"
    set_b, re_a, re_b, re_c = sc.pattern_set([pb]), sc.regex_set([ra]), sc.regex_set([rb_]), sc.regex_set([rc_, rc_])
    f_ra, f_rb, f_rc = re_filtered(all_f, ra), re_filtered(all_f, rb_), re_filtered(all_f, rc_)
    assert all(0 < len(x) < len(all_f) for x in (f_ra, f_rb, f_rc))
    try:
        # selecting from a selection is AND, whichever kind made the source
        first = res.select_device(pa)                          # a list's selection ...
        second = first.select_device(re_a)                     # ... as a regex's source
        assert 0 < len(re_filtered(filtered(all_f, pa), ra)) < len(filtered(all_f, pa))
        check_selection(sc, first.device_segments(), second, re_filtered(filtered(all_f, pa), ra), filtered(all_f, pa), ms, prints=False)
        first.free(); second.free()
        first = res.select_device(set_b)                       # a set's selection as a regex's source
        second = first.select_device(re_a)
        check_selection(sc, first.device_segments(), second, re_filtered(filtered(all_f, pb), ra), filtered(all_f, pb), ms, prints=False)
        first.free(); second.free()
        first = res.select_device(re_a)                        # and the reverse: a regex's selection as a list's and a set's source
        first_ptrs = pointers(first)
        second = first.select_device(pa)
        check_selection(sc, first.device_segments(), second, filtered(f_ra, pa), f_ra, ms, prints=False)
        assert pointers(first) == first_ptrs
        third = second.select_device(set_b)                    # it takes `first`'s block
        assert downloaded(sc, third) == filtered(filtered(f_ra, pa), pb)
        assert code_of(first.device_segments) == sx.SX_E_STATE
        first.free(); second.free(); third.free()
        # calls of the three kinds count together: valid until the second selection after it
        s1 = res.select_device(re_a)
        s2 = res.select_device(pb)
        check_selection(sc, src, s1, f_ra, all_f, ms, prints=False)                          # one selection later: still there
        assert {g[0] for g in s1.device_segments()}.isdisjoint({g[0] for g in s2.device_segments()})
        s3 = res.select_device(set_b)
        assert code_of(s1.device_segments) == sx.SX_E_STATE                                  # the third selection has taken its block
        assert code_of(lambda: s1.select_device(re_a)) == sx.SX_E_STATE
        assert code_of(lambda: s2.select_device(re_a)) == sx.SX_E_STATE                      # its block is the one this call would write
        check_selection(sc, src, s2, filtered(all_f, pb), all_f, ms, prints=False)           # (a refused call does not count)
        s1.free(); s2.free()
        s1 = res.select_device(pa)
        s2 = res.select_device(re_b)
        s4 = res.select_device(re_c)
        assert code_of(s1.device_segments) == sx.SX_E_STATE                                  # ... a list's selection after two regexes'
        check_selection(sc, src, s2, f_rb, all_f, ms, prints=False)
        assert pointers(res) == s.before
        # a selection survives a scan, and the regex set is used on the next scan's result
        s5 = res.select_device(re_c)
        res2 = sc.scan(data, file_id=1)
        assert all(g[0] is not None for g in res2.device_segments())
        p, n = s5.printed_device(n_inputs=1, radix="x")
        assert sc.download(C.c_void_p(p), n) == printed_by_python(f_rc, ms, "x", False)
        assert code_of(lambda: res.select_device(re_c)) == sx.SX_E_STATE                     # (the scan has taken the first result's memory)
        again = res2.select_device(re_c)
        ref = sx.Scanner(ms, device=0)                        # (the second buffer of a stream: its first finding may complete the last one's)
        ref.scan(data, file_id=1).free()
        host2 = ref.scan(data, file_id=1)
        all_f2 = host2.findings()
        host2.free(); ref.close()
        assert 0 < len(re_filtered(all_f2, rc_)) < len(all_f2)
        check_selection(sc, res2.device_segments(), again, re_filtered(all_f2, rc_), all_f2, ms, prints=False)
        for r in (s1, s2, s3, s4, s5, again, res2):
            r.free()
        # a regex set of another Scanner on the same device is as good as one's own
        other = sx.Scanner(ms, device=0, result_on_device=True)
        theirs = other.scan(data, file_id=1)
        sel = theirs.select_device(re_a)
        assert downloaded(other, sel) == f_ra
        sel.free(); theirs.free(); other.close()
        # what the compiler refuses arrives as SX_E_INVALID with the place
        with pytest.raises(sx.SxError) as e:
            sc.regex_set([b"ok", rb"a\b"])
        assert e.value.code == sx.SX_E_INVALID and "pattern 1, offset 1" in str(e.value)
        assert code_of(lambda: sc.regex_set([])) == sx.SX_E_INVALID
    finally:
        res.free(); sc.close()
    # the regex sets outlive the Scanner
    assert re_a.info()["n_patterns"] == 1 and re_c.info()["n_patterns"] == 2 and re_b.info()["end_states"] == 0 and re_c.info()["end_states"] == 1
    assert code_of(lambda: res.select_device(re_a)) == sx.SX_E_STATE                          # a closed Scanner
    re_a.free()
    assert code_of(re_a.info) == sx.SX_E_INVALID
    other = sx.Scanner(ms, device=0, result_on_device=True)
    theirs = other.scan(data, file_id=1)
    assert code_of(lambda: theirs.select_device(re_a)) == sx.SX_E_INVALID                     # a freed regex set
    sel = theirs.select_device(re_b)                                                           # one that has outlived its Scanner
    assert downloaded(other, sel) == f_rb
    sel.free(); theirs.free(); other.close()
    set_b.free(); re_b.free(); re_c.free()
    re_a.free()                                                                                # (twice is once)
