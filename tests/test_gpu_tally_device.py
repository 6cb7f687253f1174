"""sx_tally_set_create / sx_result_tally_device (include/stringsext_amd.h): the keyword hits of a result that lies in HBM, counted on
the device (stringsext_amd/csrc/sx_seltally_dev.hip).  As in tests/test_gpu_select_set_device.py the expected value never comes
from the code under test: a second Scanner without the flag scans the same data and Python counts in its findings by the header's
rule — hits[k] = the (finding, offset) pairs at which keyword k stands, first[k] = the smallest ordinal of such a finding.  The
keywords are taken from the data."""
import random
import struct

import pytest

import refconfig as rc
import stringsext_amd as sx
from test_gpu_result_on_device_multi import case, download_segment
from test_gpu_select_device import filtered, pick_patterns, pointers
from test_gpu_select_regex_device import re_filtered
from test_gpu_select_set_device import Source, code_of, keyword_list, seventeen
from test_host_logic import synth
from test_wave_core import text_lines

pytestmark = pytest.mark.gpu

NEVER = sx.SX_TALLY_NEVER
LDS_IDS = 4096          # the unique ids below it are counted in LDS (sx_seltally_build.hpp: kSeltallyLdsIds)


def strings(findings):
    return [f["s"].encode("utf-8") for f in findings]


def hits_by_the_rule(s, p):
    return sum(s.startswith(p, o) for o in range(len(s) - len(p) + 1))


def tally(findings, patterns, ignore_case=False, base=0):
    """(hits, first) per pattern for a short list: bytes.find from one place behind the last hit, so overlaps count"""
    strs = [s.lower() for s in strings(findings)] if ignore_case else strings(findings)
    hits, first = [], []
    for p in patterns:
        p = p.lower() if ignore_case else p
        h, f = 0, NEVER
        for i, s in enumerate(strs):
            o = s.find(p)
            if o >= 0 and f == NEVER:
                f = base + i
            while o >= 0:
                h += 1
                o = s.find(p, o + 1)
        hits.append(h); first.append(f)
    for i in range(0, len(strs), 97):           # (the rule itself, on every 97th finding)
        for p in patterns[:50]:
            p = p.lower() if ignore_case else p
            o, c = strs[i].find(p), 0
            while o >= 0:
                c, o = c + 1, strs[i].find(p, o + 1)
            assert c == hits_by_the_rule(strs[i], p)
    return hits, first


def tally_many(findings, patterns, ignore_case=False, base=0):
    """tally() for a long list of patterns of 4 bytes or more: the patterns that can begin at a place are found by its 4 bytes"""
    pats = [p.lower() for p in patterns] if ignore_case else list(patterns)
    assert all(len(p) >= 4 for p in pats)
    ids, by_head = {}, {}
    for p in pats:
        if p not in ids:
            ids[p] = len(ids)
            by_head.setdefault(p[:4], []).append(p)
    h, f = [0] * len(ids), [NEVER] * len(ids)
    for i, s in enumerate(strings(findings)):
        s = s.lower() if ignore_case else s
        here = {}
        for o in range(len(s) - 3):
            c = by_head.get(s[o:o + 4])
            if c:
                for p in c:
                    if s.startswith(p, o):
                        here[p] = here.get(p, 0) + 1
        for p, n in here.items():
            h[ids[p]] += n
            f[ids[p]] = min(f[ids[p]], base + i)
        if i % 97 == 0:
            for p in ids:                       # (the rule gives 0 exactly where Python's `in` says no)
                assert (hits_by_the_rule(s, p) if p in s else 0) == here.get(p, 0), (i, p)
    return [h[ids[p]] for p in pats], [f[ids[p]] for p in pats]


def same(got, want, patterns):
    assert got == want, [(p, g, w) for p, g, w in zip(patterns, zip(*got), zip(*want)) if g != w][:8]


def added(a, b):
    """two tallies of one stream"""
    return [x + y for x, y in zip(a[0], b[0])], [min(x, y) for x, y in zip(a[1], b[1])]


@pytest.fixture(scope="module")
def case_a():
    """case "A" — four Missions, dense: packed records, one-range strings — with its findings, keyword lists and what they count"""
    ms, data, _ = case("A")
    ref = sx.Scanner(ms, device=0)
    host = ref.scan(data, file_id=1)
    all_f = host.findings()
    host.free()
    host2 = ref.scan(data, file_id=1)           # (the second buffer of a stream: its first finding may complete the last one's)
    all_f2 = host2.findings()
    host2.free(); ref.close()
    assert len(all_f) > 1000
    kw, s17 = keyword_list(all_f), seventeen(all_f)
    return dict(ms=ms, data=data, all_f=all_f, all_f2=all_f2, seventeen=s17, keywords=kw, want17=tally(all_f, s17),
                want_kw=tally_many(all_f, kw), want_kw_nocase=tally_many(all_f, kw, ignore_case=True))


def test_several_missions_17_keywords_2000_keywords_with_decoys_and_the_fold(case_a):
    a = case_a
    s = Source(a["ms"], a["data"], all_f=a["all_f"])
    try:
        assert all(seg[4] for seg in s.src)
        n, kw = len(a["all_f"]), a["keywords"]
        ts = s.sc.tally_set(a["seventeen"])
        info = ts.info()
        assert info["n_patterns"] == 17 and info["unique"] == len(set(a["seventeen"])) and info["nocase"] == 0 and info["entry_bytes"] == 2
        assert info["states"] <= 17 * 3 + 1 and info["lds_states"] == info["states"]
        assert ts.read() == ([0] * 17, [NEVER] * 17)                                   # a new set is reset
        assert s.res.tally_device(ts) == n
        same(ts.read(), a["want17"], a["seventeen"])
        assert all(h > 0 and f < n for h, f in zip(*a["want17"]))                       # the inputs cannot hide an empty comparison
        ts.free()
        big = s.sc.tally_set(kw)
        info = big.info()
        print(info)
        assert info["n_patterns"] == len(kw) and info["unique"] == len(set(kw)) and info["states"] > info["lds_states"] > 0
        assert info["states"] == len({p[:k] for p in kw for k in range(len(p) + 1)}) and info["entry_bytes"] == (2 if info["states"] <= 32768 else 4)
        assert info["table_bytes"] == 256 + info["states"] * info["classes"] * info["entry_bytes"] + 8 * info["states"] + 4 * len(kw)
        assert s.res.tally_device(big) == n
        got = big.read()
        same(got, a["want_kw"], kw)
        decoys = [k for k, p in enumerate(kw) if p[:1] == b"\x02"]
        assert len(decoys) == len(kw) // 2 and all((got[0][k], got[1][k]) == (0, NEVER) for k in decoys)
        assert all(got[0][k] > 0 for k in range(len(kw)) if k not in set(decoys))
        big.free()
        folded = s.sc.tally_set(kw, ignore_case=True)
        assert folded.info()["nocase"] == 1 and folded.info()["unique"] == len({p.lower() for p in kw})
        s.res.tally_device(folded)
        got = folded.read()
        same(got, a["want_kw_nocase"], kw)
        assert all(x >= y for x, y in zip(got[0], a["want_kw"][0])) and sum(got[0]) > sum(a["want_kw"][0])
        folded.free()
    finally:
        s.close()


def test_a_hot_keyword_next_to_rare_ones_on_both_sides_of_the_lds_counters():
    """one byte that most findings hold — counted in the workgroups' LDS counters and flushed — next to more than 4096 other
    keywords, the longest of which have the ids that are counted in HBM at once.  The data is text alone, two Missions merged: lines
    of 10..119 letters out of 53, so a given letter stands in about two lines of three (in case "A", with its short findings out of
    random bytes and UTF-16, no byte stands in half of the findings)"""
    s = Source(rc.missions(encodings=["ascii", "utf-8"], chars_min="5"), text_lines(random.Random(79), 1_500_000))
    try:
        all_f, strs = s.all_f, strings(s.all_f)
        assert len(strs) > 10000
        holds = {}
        for x in strs:
            for b in set(x):
                holds[b] = holds.get(b, 0) + 1
        hot = bytes([max(holds, key=lambda b: (holds[b], b))])
        assert holds[hot[0]] > len(strs) // 2
        rare = keyword_list(all_f, n=3000)
        pats = rare[:1500] + [hot] + rare[1500:]
        ts = s.sc.tally_set(pats)
        assert ts.info()["unique"] > LDS_IDS + 100
        assert s.res.tally_device(ts) == len(all_f)
        got = ts.read()
        want = tally_many(all_f, rare)
        want_hot = tally(all_f, [hot])
        print(f"{len(strs)} findings; {hot!r} stands in {holds[hot[0]]} of them, {want_hot[0][0]} times")
        assert (got[0][1500], got[1][1500]) == (want_hot[0][0], want_hot[1][0]) and want_hot[0][0] >= holds[hot[0]]
        same((got[0][:1500] + got[0][1501:], got[1][:1500] + got[1][1501:]), want, rare)
        # which side counted what: the map from pattern to unique id, where it lies
        d_hits, d_first, d_map, unique = ts.counters_device()
        ids = struct.unpack(f"<{len(pats)}I", s.sc.download(d_map, 4 * len(pats)))
        assert ids[1500] < LDS_IDS                                                     # one byte: the first state below the root
        assert sum(1 for k, u in enumerate(ids) if u >= LDS_IDS and got[0][k] > 0) > 50 and sum(1 for k, u in enumerate(ids) if u < LDS_IDS and got[0][k] > 0) > 50
        ts.free()
    finally:
        s.close()


def test_counters_where_they_lie_expand_to_what_read_returns(case_a):
    a = case_a
    s = Source(a["ms"], a["data"], all_f=a["all_f"])
    try:
        pats = a["seventeen"] + a["seventeen"][:5] + [p.upper() for p in a["seventeen"][:3]]
        ts = s.sc.tally_set(pats, ignore_case=True)
        s.res.tally_device(ts, ordinal_base=10)
        d_hits, d_first, d_map, unique = ts.counters_device()
        assert unique == ts.info()["unique"] == len({p.lower() for p in pats}) < len(pats)
        hits = struct.unpack(f"<{unique}Q", s.sc.download(d_hits, 8 * unique))
        first = struct.unpack(f"<{unique}Q", s.sc.download(d_first, 8 * unique))
        ids = struct.unpack(f"<{len(pats)}I", s.sc.download(d_map, 4 * len(pats)))
        assert sorted(set(ids)) == list(range(unique))
        assert ([hits[u] for u in ids], [first[u] for u in ids]) == ts.read()
        same(ts.read(), tally(a["all_f"], pats, ignore_case=True, base=10), pats)
        ts.free()
    finally:
        s.close()


def test_unpacked_merger_records(monkeypatch, case_a):
    monkeypatch.setenv("SX_PACKED", "0")
    a = case_a
    s = Source(a["ms"], a["data"], all_f=a["all_f"])
    try:
        assert all(not seg[4] for seg in s.src)
        ts, big = s.sc.tally_set(a["seventeen"]), s.sc.tally_set(a["keywords"])
        assert s.res.tally_device(ts) == s.res.tally_device(big) == len(a["all_f"])
        same(ts.read(), a["want17"], a["seventeen"])
        same(big.read(), a["want_kw"], a["keywords"])
        ts.free(); big.free()
    finally:
        s.close()


def test_several_parts_are_several_segments_and_first_is_the_ordinal_across_them(monkeypatch, case_a):
    monkeypatch.setenv("SX_MERGE_PART_FINDINGS", "7000")
    monkeypatch.setenv("SX_MERGE_PART_MIB", "1")
    a = case_a
    s = Source(a["ms"], a["data"], all_f=a["all_f"])
    try:
        assert len(s.src) >= 3
        ts, big = s.sc.tally_set(a["seventeen"]), s.sc.tally_set(a["keywords"], ignore_case=True)
        assert s.res.tally_device(ts, ordinal_base=1 << 40) == len(a["all_f"])
        want = tally(a["all_f"], a["seventeen"], base=1 << 40)
        assert all(f >= 1 << 40 for f in want[1])
        same(ts.read(), want, a["seventeen"])
        s.res.tally_device(big)
        same(big.read(), a["want_kw_nocase"], a["keywords"])
        assert max(f for f in a["want_kw_nocase"][1] if f != NEVER) >= s.src[0][1] + s.src[1][1]        # some keyword shows first in the third segment or behind
        ts.free(); big.free()
    finally:
        s.close()


def one_mission(ms, data, device_replay, packed):
    s = Source(ms, data, device_replay=device_replay)
    try:
        assert len(s.all_f) >= 100 and all(seg[4] == packed for seg in s.src)
        pats = seventeen(s.all_f) + [b"\x02never"]
        want = tally(s.all_f, pats, base=5)
        print(f"{len(s.all_f)} findings, hits {want[0]}")
        assert all(h > 0 for h in want[0][:17]) and (want[0][17], want[1][17]) == (0, NEVER)
        ts = s.sc.tally_set(pats)
        assert s.res.tally_device(ts, ordinal_base=5) == len(s.all_f)
        same(ts.read(), want, pats)
        ts.free()
    finally:
        s.close()


def test_one_mission_dense_packed_segment(monkeypatch):
    """the wave path's segment: sx_finding16 records, strings where the writer put them"""
    monkeypatch.setenv("SX_WAVE_REPLAY", "1")
    data = text_lines(random.Random(77), 3_000_000)
    one_mission(rc.missions(encodings=["ascii"], chars_min="4"), data, None, True)


def test_one_mission_sparse_unpacked_segment():
    """the lane-per-region replay's segment: sx_finding records"""
    data = synth(random.Random(78), 8_000_000, 1 / 400)
    one_mission(rc.missions(encodings=["utf-8"], chars_min="10"), data, True, False)


def test_calls_add_up_reset_forgets_and_a_second_buffer_goes_on_counting(case_a):
    a = case_a
    s = Source(a["ms"], a["data"], all_f=a["all_f"])
    try:
        n, pats, want = len(a["all_f"]), a["seventeen"], a["want17"]
        ts = s.sc.tally_set(pats)
        assert s.res.tally_device(ts, ordinal_base=0) == n
        assert s.res.tally_device(ts, ordinal_base=len(s.res)) == n                    # the same result again, behind itself
        same(ts.read(), ([2 * h for h in want[0]], want[1]), pats)
        ts.reset()
        assert ts.read() == ([0] * 17, [NEVER] * 17)
        # the stream's second buffer on the same Scanner, into the same set
        s.res.tally_device(ts)
        res2 = s.sc.scan(a["data"], file_id=1)
        assert len(res2) == len(a["all_f2"]) and all(g[0] is not None for g in res2.device_segments())
        assert res2.tally_device(ts, ordinal_base=n) == len(a["all_f2"])
        same(ts.read(), tally(a["all_f"] + a["all_f2"], pats), pats)
        # ... and a keyword that only the second buffer's tally could have seen first keeps the stream's ordinal
        ts.reset()
        res2.tally_device(ts, ordinal_base=n)
        same(ts.read(), tally(a["all_f2"], pats, base=n), pats)
        res2.free(); ts.free()
    finally:
        s.res.free(); s.sc.close()


def test_selections_of_all_three_kinds_are_sources_and_a_tally_ages_none(case_a):
    a = case_a
    all_f = a["all_f"]
    s = Source(a["ms"], a["data"], all_f=all_f)
    sc, res = s.sc, s.res
    try:
        sets = pick_patterns(all_f)
        pa, pb, pc = sets["one"][0], sets["three"][0], sets["eight"][0]
        pats = a["seventeen"] + [pa, pb]
        ts = sc.tally_set(pats)
        shape = rb"[0-9]{3}\.[0-9]"
        ps, rs = sc.pattern_set([pb, pc]), sc.regex_set([shape])
        for how, kept in ((pa, filtered(all_f, pa)), (ps, filtered(all_f, [pb, pc])), (rs, re_filtered(all_f, [shape]))):
            assert 0 < len(kept) < len(all_f)
            sel = res.select_device(how)
            before = pointers(sel)
            assert sel.tally_device(ts, ordinal_base=3) == len(kept)
            same(ts.read(), tally(kept, pats, base=3), pats)
            assert pointers(sel) == before and pointers(res) == s.before               # read, not moved
            ts.reset(); sel.free()
        # a tally between two selections does not count as one: s1 goes stale only after the SECOND selection behind it
        s1 = res.select_device(pa)
        s1.tally_device(ts); res.tally_device(ts)
        s2 = res.select_device(ps)
        s1.tally_device(ts); s2.tally_device(ts); res.tally_device(ts)
        ts.reset()
        assert s1.tally_device(ts) == len(filtered(all_f, pa))                          # select, tally, select: still there
        same(ts.read(), tally(filtered(all_f, pa), pats), pats)
        assert s1.device_segments()
        s3 = res.select_device(rs)
        ts.reset()
        assert code_of(lambda: s1.tally_device(ts)) == sx.SX_E_STATE                    # the third selection has taken its block
        assert ts.read() == ([0] * len(pats), [NEVER] * len(pats))
        assert s2.tally_device(ts) == len(filtered(all_f, [pb, pc])) and s3.tally_device(ts) == len(re_filtered(all_f, [shape]))
        for r in (s1, s2, s3):
            r.free()
        ts.free(); ps.free(); rs.free()
    finally:
        s.close()


def test_a_keyword_that_spans_two_findings_counts_nothing(case_a):
    a = case_a
    s = Source(a["ms"], a["data"], all_f=a["all_f"])
    try:
        recs, arena = download_segment(s.sc, s.src[0])
        strs = strings(a["all_f"][:s.src[0][1]])
        assert b"".join(strs) == arena                                             # back to back: neighbours in the list are neighbours in HBM
        everywhere = strings(a["all_f"])
        spans = []
        for i in range(0, len(strs) - 1, max(1, len(strs) // 200)):
            p = strs[i][-3:] + strs[i + 1][:3]
            if not any(p in x for x in everywhere):
                spans.append(p)
            if len(spans) == 40:
                break
        assert spans and all(p in arena for p in spans)
        pats = spans + [a["seventeen"][0]]
        ts = s.sc.tally_set(pats)
        s.res.tally_device(ts)
        assert ts.read() == ([0] * len(spans) + [a["want17"][0][0]], [NEVER] * len(spans) + [a["want17"][1][0]])
        ts.free()
    finally:
        s.close()


def test_refused_sources_add_nothing_and_the_set_outlives_its_scanner(case_a):
    a = case_a
    all_f, pats = a["all_f"], a["seventeen"]
    s = Source(a["ms"], a["data"], all_f=all_f)
    sc, res = s.sc, s.res
    try:
        ts = sc.tally_set(pats)
        res.tally_device(ts, ordinal_base=9)
        want = tally(all_f, pats, base=9)
        # an empty selection is in host memory, as every result without findings
        none = res.select_device(b"\x02\x02")
        assert len(none) == 0 and code_of(lambda: none.tally_device(ts)) == sx.SX_E_STATE
        none.free()
        # a host result of a Scanner without the flag
        plain = sx.Scanner(a["ms"], device=0)
        host = plain.scan(a["data"], file_id=1)
        assert code_of(lambda: host.tally_device(ts)) == sx.SX_E_STATE
        host.free(); plain.close()
        # a result whose memory a later scan took
        res2 = sc.scan(a["data"], file_id=1)
        assert code_of(lambda: res.tally_device(ts)) == sx.SX_E_STATE
        same(ts.read(), want, pats)                                                     # nothing of all that was added
        assert res2.tally_device(ts, ordinal_base=len(all_f) + 9) == len(a["all_f2"])
        same(ts.read(), added(want, tally(a["all_f2"], pats, base=len(all_f) + 9)), pats)
        # a freed set
        gone = sc.tally_set(pats)
        gone.free(); gone.free()
        assert code_of(lambda: res2.tally_device(gone)) == sx.SX_E_INVALID and code_of(gone.read) == sx.SX_E_INVALID
        res2.free()
    finally:
        res.free(); sc.close()
    # a closed Scanner; the set is still there ...
    assert code_of(lambda: res.tally_device(ts)) == sx.SX_E_STATE
    assert ts.info()["n_patterns"] == 17
    ts.reset()
    # ... and another Scanner on the same device counts into it
    other = sx.Scanner(a["ms"], device=0, result_on_device=True)
    theirs = other.scan(a["data"], file_id=1)
    assert theirs.tally_device(ts) == len(all_f)
    same(ts.read(), a["want17"], pats)
    theirs.free(); other.close()
    same(ts.read(), a["want17"], pats)
    ts.free()
