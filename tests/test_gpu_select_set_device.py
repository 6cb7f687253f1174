"""sx_select_set_create / sx_result_select_set_device (include/stringsext_amd.h): the findings of a result that lies in HBM, selected
by a compiled keyword list on the device (stringsext_amd/csrc/sx_selset_dev.hip).  As in tests/test_gpu_select_device.py the
expected value never comes from the code under test: a second Scanner without the flag scans the same data and Python filters
its findings with the header's match rule.  The keywords are taken from the data."""
import ctypes as C
import random

import pytest

import refconfig as rc
import stringsext_amd as sx
import sxo_binding as sxo
from test_gpu_result_on_device_multi import case, download_segment
from test_gpu_select_device import check_selection, downloaded, filtered, matches, middle3, pick_patterns, pointers, printed_by_python
from test_host_logic import synth
from test_wave_core import text_lines

pytestmark = pytest.mark.gpu


def code_of(call):
    with pytest.raises(sx.SxError) as e:
        call()
    return e.value.code


def seventeen(findings):
    """one pattern more than the list selection takes"""
    strs = [f["s"].encode("utf-8") for f in findings]
    return [middle3(strs[k * len(strs) // 17]) for k in range(17)]


def keyword_list(findings, n=2000):
    """the middle 4..10 bytes of every k-th string (of those that have four: the cut-off tail of a string may have fewer), and as
    many decoys that occur nowhere (no finding holds a control byte)"""
    strs = [f["s"].encode("utf-8") for f in findings]
    assert not any(b"\x02" in s for s in strs)
    strs = [s for s in strs if len(s) >= 4]
    pats = []
    for i, s in enumerate(strs[::max(1, len(strs) // n)][:n]):
        ln = min(len(s), 4 + i % 7)
        pats.append(s[(len(s) - ln) // 2:(len(s) - ln) // 2 + ln])
    assert all(len(p) >= 4 for p in pats)
    return pats + [b"\x02" + p for p in pats]


def filtered_many(findings, patterns, ignore_case=False, invert=False):
    """filtered() for a long list of patterns of 4 bytes or more: the patterns that can begin at a place are found by its 4 bytes"""
    if ignore_case:
        patterns = [p.lower() for p in patterns]
    by_head = {}
    for p in patterns:
        by_head.setdefault(p[:4], []).append(p)

    def hit(s):
        s = s.lower() if ignore_case else s
        for o in range(len(s) - 3):
            c = by_head.get(s[o:o + 4])
            if c and any(s.startswith(p, o) for p in c):
                return True
        return False
    out = [f for f in findings if hit(f["s"].encode("utf-8")) != invert]
    ids = {id(f) for f in out}
    for f in findings[::97]:        # (the same rule as filtered()'s)
        assert (matches(f["s"].encode("utf-8"), patterns, ignore_case) != invert) == (id(f) in ids)
    return out


class Source:
    """a case scanned twice: the findings of a Scanner without the flag, and the result that stays on the device"""

    def __init__(self, ms, data, device_replay=None, all_f=None):
        self.ms, self.data = ms, data
        if all_f is None:
            ref = sx.Scanner(ms, device=0, device_replay=device_replay)
            host = ref.scan(data, file_id=1)
            all_f = host.findings()
            host.free(); ref.close()
        self.all_f = all_f
        self.sc = sx.Scanner(ms, device=0, device_replay=device_replay, result_on_device=True)
        self.res = self.sc.scan(data, file_id=1)
        self.src = self.res.device_segments()
        assert all(s[0] is not None for s in self.src) and sum(s[1] for s in self.src) == len(all_f)
        self.before = pointers(self.res)

    def check(self, ps, want, invert=False, prints=False):
        sel = self.res.select_device(ps, invert=invert)
        check_selection(self.sc, self.src, sel, want, self.all_f, self.ms, prints=prints)
        sel.free()

    def close(self):
        assert pointers(self.res) == self.before          # the source was read, not moved
        self.res.free(); self.sc.close()


@pytest.fixture(scope="module")
def case_a():
    """case "A" — four Missions, dense: packed records, one-range strings — with its findings and keyword lists"""
    ms, data, _ = case("A")
    ref = sx.Scanner(ms, device=0)
    host = ref.scan(data, file_id=1)
    all_f = host.findings()
    host.free(); ref.close()
    assert len(all_f) > 1000
    kw = keyword_list(all_f)
    return dict(ms=ms, data=data, all_f=all_f, seventeen=seventeen(all_f), keywords=kw,
                want17=filtered(all_f, seventeen(all_f)), want_kw=filtered_many(all_f, kw), want_kw_nocase=filtered_many(all_f, kw, ignore_case=True))


def test_several_missions_17_patterns_and_2000_keywords(case_a):
    a = case_a
    s = Source(a["ms"], a["data"], all_f=a["all_f"])
    try:
        assert all(seg[4] for seg in s.src)
        n = len(a["all_f"])
        print(f"{n} findings; 17 patterns select {len(a['want17'])}, {len(a['keywords'])} keywords {len(a['want_kw'])}, folded {len(a['want_kw_nocase'])}")
        assert 0 < len(a["want17"]) < n and 0 < len(a["want_kw"]) < n and 0 < len(a["want_kw_nocase"]) < n
        assert len(a["want_kw_nocase"]) >= len(a["want_kw"])
        ps = s.sc.pattern_set(a["seventeen"])
        info = ps.info()
        assert info["n_patterns"] == 17 and info["nocase"] == 0 and info["states"] <= 17 * 3 + 2 and info["lds_states"] == info["states"]
        s.check(ps, a["want17"], prints=True)
        ps.free()
        big = s.sc.pattern_set(a["keywords"])
        info = big.info()
        print(info)
        assert info["n_patterns"] == len(a["keywords"]) and info["states"] > info["lds_states"] > 0 and info["classes"] <= 256
        assert info["table_bytes"] >= info["states"] * info["classes"] * 2
        s.check(big, a["want_kw"])
        big.free()
        folded = s.sc.pattern_set(a["keywords"], ignore_case=True)
        assert folded.info()["nocase"] == 1 and folded.info()["states"] > folded.info()["lds_states"]
        s.check(folded, a["want_kw_nocase"])
        with pytest.raises(ValueError):
            s.res.select_device(folded, ignore_case=True)
        folded.free()
        assert code_of(lambda: s.res.select_device(folded)) == sx.SX_E_INVALID         # a freed set
    finally:
        s.close()


def test_the_set_and_the_list_agree_on_sixteen_patterns(case_a):
    a = case_a
    s = Source(a["ms"], a["data"], all_f=a["all_f"])
    try:
        for name in ("sixteen", "three", "two nocase"):
            pats, nocase = pick_patterns(a["all_f"])[name]
            pats = [pats] if isinstance(pats, bytes) else pats
            ps = s.sc.pattern_set(pats, ignore_case=nocase)
            by_set, by_list = s.res.select_device(ps), s.res.select_device(pats, ignore_case=nocase)
            assert 0 < len(by_set) == len(by_list) < len(a["all_f"])
            assert [(g[1], g[3], g[4]) for g in by_set.device_segments()] == [(g[1], g[3], g[4]) for g in by_list.device_segments()]
            assert downloaded(s.sc, by_set) == downloaded(s.sc, by_list) == filtered(a["all_f"], pats, nocase)
            by_set.free(); by_list.free(); ps.free()
    finally:
        s.close()


def test_invert_partitions_the_source_and_nothing_and_everything(case_a):
    a = case_a
    s = Source(a["ms"], a["data"], all_f=a["all_f"])
    try:
        ps = s.sc.pattern_set(a["seventeen"])
        plain, inverse = s.res.select_device(ps), s.res.select_device(ps, invert=True)
        assert len(plain) + len(inverse) == len(s.res) and len(plain) and len(inverse)
        check_selection(s.sc, s.src, inverse, filtered(a["all_f"], a["seventeen"], invert=True), a["all_f"], a["ms"], prints=False)
        check_selection(s.sc, s.src, plain, a["want17"], a["all_f"], a["ms"], prints=False)
        plain.free(); inverse.free(); ps.free()
        decoys = s.sc.pattern_set([p for p in a["keywords"] if p[:1] == b"\x02"])
        none = s.res.select_device(decoys)
        assert len(none) == 0 and none.device_segments() == [] and none.segments() == [] and none.findings() == []
        assert code_of(lambda: none.select_device(decoys)) == sx.SX_E_STATE        # an empty result is in host memory
        everything = s.res.select_device(decoys, invert=True)
        check_selection(s.sc, s.src, everything, a["all_f"], a["all_f"], a["ms"], prints=False)
        none.free(); everything.free(); decoys.free()
    finally:
        s.close()


def test_a_keyword_that_spans_two_findings_selects_nothing(case_a):
    a = case_a
    s = Source(a["ms"], a["data"], all_f=a["all_f"])
    try:
        recs, arena = download_segment(s.sc, s.src[0])
        strs = [f["s"].encode("utf-8") for f in a["all_f"][:s.src[0][1]]]
        assert b"".join(strs) == arena                                             # back to back: neighbours in the list are neighbours in HBM
        everywhere = [f["s"].encode("utf-8") for f in a["all_f"]]
        spans = []
        for i in range(0, len(strs) - 1, max(1, len(strs) // 200)):
            p = strs[i][-3:] + strs[i + 1][:3]
            if not any(p in x for x in everywhere):
                spans.append(p)
            if len(spans) == 40:
                break
        assert spans and all(p in arena for p in spans)
        ps = s.sc.pattern_set(spans)
        sel = s.res.select_device(ps)
        assert len(sel) == 0 and sel.device_segments() == []
        sel.free()
        # ... and with a keyword that does occur among them, exactly its findings
        ps2 = s.sc.pattern_set(spans + [a["seventeen"][0]])
        s.check(ps2, filtered(a["all_f"], a["seventeen"][0]))
        ps.free(); ps2.free()
    finally:
        s.close()


def test_unpacked_merger_records(monkeypatch, case_a):
    monkeypatch.setenv("SX_PACKED", "0")
    a = case_a
    s = Source(a["ms"], a["data"], all_f=a["all_f"])
    try:
        assert all(not seg[4] for seg in s.src)
        ps, big = s.sc.pattern_set(a["seventeen"]), s.sc.pattern_set(a["keywords"])
        s.check(ps, a["want17"])
        s.check(ps, filtered(a["all_f"], a["seventeen"], invert=True), invert=True)
        s.check(big, a["want_kw"])
        ps.free(); big.free()
    finally:
        s.close()


def test_several_parts_are_several_segments(monkeypatch, case_a):
    monkeypatch.setenv("SX_MERGE_PART_FINDINGS", "7000")
    monkeypatch.setenv("SX_MERGE_PART_MIB", "1")
    a = case_a
    s = Source(a["ms"], a["data"], all_f=a["all_f"])
    try:
        assert len(s.src) >= 3
        ps, big = s.sc.pattern_set(a["seventeen"]), s.sc.pattern_set(a["keywords"], ignore_case=True)
        s.check(ps, a["want17"])
        s.check(big, a["want_kw_nocase"])
        sel = s.res.select_device(big)
        assert len(sel.device_segments()) >= 3
        sel.free(); ps.free(); big.free()
    finally:
        s.close()


def one_mission(ms, data, device_replay, packed):
    s = Source(ms, data, device_replay=device_replay)
    try:
        assert len(s.all_f) >= 100 and all(seg[4] == packed for seg in s.src)
        pats = seventeen(s.all_f)
        want = filtered(s.all_f, pats)
        print(f"17 patterns select {len(want)} of {len(s.all_f)}")
        assert 0 < len(want) < len(s.all_f)
        ps = s.sc.pattern_set(pats)
        s.check(ps, want)
        s.check(ps, filtered(s.all_f, pats, invert=True), invert=True)
        ps.free()
        return len(s.src)
    finally:
        s.close()


def test_one_mission_dense_packed_segment(monkeypatch):
    """the wave path's segment: sx_finding16 records, strings where the writer put them"""
    monkeypatch.setenv("SX_WAVE_REPLAY", "1")
    data = text_lines(random.Random(77), 3_000_000)
    assert one_mission(rc.missions(encodings=["ascii"], chars_min="4"), data, None, True) == 1


def test_one_mission_sparse_unpacked_segment():
    """the lane-per-region replay's segment: sx_finding records"""
    data = synth(random.Random(78), 8_000_000, 1 / 400)
    one_mission(rc.missions(encodings=["utf-8"], chars_min="10"), data, True, False)


def test_composition_and_lifetime(case_a):
    a = case_a
    ms, data, all_f = a["ms"], a["data"], a["all_f"]
    want_text = sxo.run_cli(ms, [data], radix="x")
    s = Source(ms, data, all_f=all_f)
    sc, res, src = s.sc, s.res, s.src
    sets = pick_patterns(all_f)
    pa, pb, pc = sets["one"][0], sets["three"][0], sets["eight"][0]
    set_a, set_b, set_c = sc.pattern_set([pa]), sc.pattern_set([pb], ignore_case=True), sc.pattern_set([pc, pc])
    try:
        # selecting from a selection is AND, whichever kind made the source
        both = filtered(filtered(all_f, pa), pb, ignore_case=True)
        assert 0 < len(both) < len(filtered(all_f, pa))
        first = res.select_device(pa)                          # a list's selection ...
        second = first.select_device(set_b)                    # ... as a set's source
        check_selection(sc, first.device_segments(), second, both, filtered(all_f, pa), ms, prints=False)
        first.free(); second.free()
        first = res.select_device(set_b)                       # and the other way round
        first_ptrs = pointers(first)
        second = first.select_device(pa)
        check_selection(sc, first.device_segments(), second, filtered(filtered(all_f, pb, ignore_case=True), pa), filtered(all_f, pb, ignore_case=True), ms, prints=False)
        assert pointers(first) == first_ptrs
        third = second.select_device(set_a)                    # a set over a list's selection out of a set's; it takes `first`'s block
        assert downloaded(sc, third) == filtered(filtered(all_f, pb, ignore_case=True), pa)
        assert code_of(first.device_segments) == sx.SX_E_STATE
        first.free(); second.free(); third.free()
        # calls of both kinds count together: valid until the second selection after it
        s1 = res.select_device(set_a)
        s2 = res.select_device(pb)
        check_selection(sc, src, s1, filtered(all_f, pa), all_f, ms, prints=False)          # one selection later: still there
        assert {g[0] for g in s1.device_segments()}.isdisjoint({g[0] for g in s2.device_segments()})
        s3 = res.select_device(set_c)
        assert code_of(s1.device_segments) == sx.SX_E_STATE                                  # the third selection has taken its block
        assert code_of(lambda: s1.select_device(set_a)) == sx.SX_E_STATE
        assert code_of(lambda: s1.printed_device(radix="x")) == sx.SX_E_STATE
        assert code_of(lambda: s2.select_device(set_a)) == sx.SX_E_STATE                     # its block is the one this call would write
        check_selection(sc, src, s2, filtered(all_f, pb), all_f, ms, prints=False)           # (a refused call does not count)
        s1.free(); s2.free()
        s1 = res.select_device(pa)
        s2 = res.select_device(set_b)
        s4 = res.select_device(pc)
        assert code_of(s1.device_segments) == sx.SX_E_STATE                                  # ... a list's selection after a set's and a list's
        check_selection(sc, src, s2, filtered(all_f, pb, ignore_case=True), all_f, ms, prints=False)
        # the source is where it was and still prints the oracle's full text
        assert pointers(res) == s.before
        p, n = res.printed_device(n_inputs=1, radix="x")
        assert sx.OUTPUT_BOM + sc.download(C.c_void_p(p), n) + b"\n" == want_text
        # a selection survives a scan, and the set is used on the next scan's result
        s5 = res.select_device(set_c)
        res2 = sc.scan(data, file_id=1)
        assert all(g[0] is not None for g in res2.device_segments())
        p, n = s5.printed_device(n_inputs=1, radix="x")
        assert sc.download(C.c_void_p(p), n) == printed_by_python(filtered(all_f, pc), ms, "x", False)
        assert code_of(lambda: res.select_device(set_c)) == sx.SX_E_STATE                    # (the scan has taken the first result's memory)
        again = res2.select_device(set_c)
        ref = sx.Scanner(ms, device=0)                        # (the second buffer of a stream: its first finding may complete the last one's)
        ref.scan(data, file_id=1).free()
        host2 = ref.scan(data, file_id=1)
        all_f2 = host2.findings()
        host2.free(); ref.close()
        assert 0 < len(filtered(all_f2, pc)) < len(all_f2)
        check_selection(sc, res2.device_segments(), again, filtered(all_f2, pc), all_f2, ms, prints=False)
        for r in (s1, s2, s3, s4, s5, again, res2):
            r.free()
        # a set of another Scanner on the same device is as good as one's own
        other = sx.Scanner(ms, device=0, result_on_device=True)
        theirs = other.scan(data, file_id=1)
        sel = theirs.select_device(set_a)
        assert downloaded(other, sel) == filtered(all_f, pa)
        sel.free(); theirs.free(); other.close()
    finally:
        res.free(); sc.close()
    # the sets outlive the Scanner
    assert set_a.info()["n_patterns"] == 1 and set_c.info()["n_patterns"] == 2 and set_b.info()["nocase"] == 1
    assert code_of(lambda: res.select_device(set_a)) == sx.SX_E_STATE                         # a closed Scanner
    set_a.free(); set_b.free(); set_c.free()
    set_a.free()                                                                              # (twice is once)
