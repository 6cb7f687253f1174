"""sx_extract_regex_create / sx_result_extract_regex_device (include/stringsext_amd.h): the regex matches of a result that lies in
HBM, cut out on the device (stringsext_amd/csrc/sx_extract_dev.hip).  The expected value never comes from the code under test: a
second Scanner without the flag scans the same data, and the brute force over Python's `re` of tests/test_extract_core.py says where
the matches of every finding's string lie — in front of it one more question to the same engine, "does the pattern, followed by
anything, match at this offset at all", which only spares the offsets where the brute force would try every end in vain."""
import ctypes as C
import functools
import random
import re

import pytest

import refconfig as rc
import stringsext_amd as sx
from test_extract_core import ends_at, matches
from test_gpu_result_on_device_multi import case
from test_gpu_select_device import downloaded, info_tuple, pointers, printed_by_python
from test_gpu_select_set_device import Source, code_of
from test_host_logic import synth
from test_selre_core import to_python

pytestmark = pytest.mark.gpu

URL, MAIL, QUAD = rb"https?://[a-z0-9./_-]+", rb"[a-z0-9._]+@[a-z0-9-]+(\.[a-z0-9-]+)+", rb"([0-9]{1,3}\.){3}[0-9]{1,3}"


@functools.lru_cache(maxsize=None)
def begins_at(p, nocase):
    return re.compile(b"(?:" + to_python(p) + b")(?s:.*)\\Z", re.IGNORECASE if nocase else 0)


def oracle(patterns, nocase, s):
    out, o, n = [], 0, len(s)
    while o < n:
        e = None
        if any(begins_at(p, nocase).match(s, o) for p in patterns):
            e = next((e for e in range(n, o, -1) if any(ends_at(p, n - e, nocase).match(s, o) for p in patterns)), None)
        if e is None:
            o += 1
        else:
            out.append((o, e)); o = e
    return out


def test_the_spared_offsets_change_nothing():
    rng = random.Random(5)
    for _ in range(200):
        s = bytes(rng.choice(b"ab.@1/:h tp") for _ in range(rng.randrange(0, 40)))
        for pats in ([URL, MAIL, QUAD], [b"a*b|^b", b"1+$"], [b"a*"]):
            assert oracle(pats, False, s) == matches(pats, False, s)


def expected(findings, pats, nocase=False):
    """(the findings the extraction must give, the matches per source finding)"""
    out, per = [], []
    for f in findings:
        s = f["s"].encode("utf-8")
        ms = oracle(tuple(pats), nocase, s)
        per.append(len(ms))
        out += [dict(f, s=s[o:e].decode("utf-8")) for o, e in ms]      # every field the finding's, but the string
    return out, per


def check_extraction(sc, src_segs, ext, want, per, ms, prints=False):
    assert len(ext) == len(want)
    segs = ext.device_segments()
    at, expect = 0, []      # every source segment with a match gives one segment: its record type, its sx_segment_info
    for s in src_segs:
        k = sum(per[at:at + s[1]])
        at += s[1]
        if k:
            expect.append((k, s[4], info_tuple(s[5])))
    assert at == len(per)
    assert [(s[1], s[4], info_tuple(s[5])) for s in segs] == expect
    got = downloaded(sc, ext)      # (checks the layout: 256-byte aligned, [records][strings], the strings back to back in record order)
    assert got == want, next(((a, b) for a, b in zip(got, want) if a != b), (len(got), len(want)))
    if prints:
        p, n = ext.printed_device(n_inputs=1, radix="x")
        text = sc.download(C.c_void_p(p), n)
        assert text == printed_by_python(want, ms, "x", False) == ext.printed(n_inputs=1, radix="x")
        assert ext.findings() == want


def extract_and_check(s, pats, nocase=False, prints=False):
    want, per = expected(s.all_f, pats, nocase)
    xs = s.sc.extract_set(pats, ignore_case=nocase)
    info = xs.info()
    assert info["n_patterns"] == len(pats) and info["nocase"] == int(nocase) and info["table_bytes"] == info["states"] * info["classes"] * 2
    ext = s.res.extract_device(xs)
    check_extraction(s.sc, s.src, ext, want, per, s.ms, prints=prints)
    ext.free(); xs.free()
    return want, per


def planted(rng, n_lines=3500):
    """text lines with known numbers of URLs, e-mail addresses and dotted quads; every eighth line in UTF-16LE"""
    words = [b"alpha", b"bravo", b"charlie", b"delta", b"echo", b"foxtrot", b"golf", b"hotel"]
    def url(): return b"http%s://%s.example.org/%s_%d" % (rng.choice((b"", b"s")), rng.choice(words), rng.choice(words), rng.randrange(100))
    def mail(): return b"%s.%d@%s-mail.example.com" % (rng.choice(words), rng.randrange(100), rng.choice(words))
    def quad(): return b"%d.%d.%d.%d" % tuple(rng.randrange(256) for _ in range(4))
    lines, counts = [], []
    for i in range(n_lines):
        k = (0, 0, 1, 1, 2, 3, 4)[i % 7]
        parts = [rng.choice(words) for _ in range(rng.randrange(2, 6))]
        hits = [rng.choice((url, mail, quad))() for _ in range(k)]
        for h in hits:
            parts.insert(rng.randrange(len(parts) + 1), h)
        if k and i % 5 == 0:
            parts = [hits[0]] + [p for p in parts if p is not hits[0]]      # a match at the line's first byte
        if k and i % 5 == 1:
            parts = [p for p in parts if p is not hits[-1]] + [hits[-1]]    # ... and at its last
        line = b" ".join(parts)
        if i % 8 == 7:      # (in front of it a U+0000, which ends whatever the UTF-16 Mission has made of the ASCII lines)
            lines.append(b"\x00\x00" + line.decode().encode("utf-16le") + b"\n\x00")
        else:               # (an even number of bytes: the UTF-16 lines stay aligned)
            lines.append(line + (b"\n" if len(line) % 2 else b" \n"))
        counts.append(k)
    return b"".join(lines), counts


@pytest.fixture(scope="module")
def planted_source():
    data, counts = planted(random.Random(2027))
    assert 150_000 < len(data) < 600_000
    s = Source(rc.missions(encodings=["utf-8", "utf-16le"], chars_min="5"), data)
    s.counts = counts
    yield s
    s.close()


def test_a_planted_buffer_of_urls_addresses_and_quads(planted_source):
    s = planted_source
    assert all(seg[4] for seg in s.src)                                   # two Missions: packed records, strings one range
    pats = [URL, MAIL, QUAD]
    want, per = expected(s.all_f, pats)
    # the planted counts make the comparison say something, by construction — asserted before anything is compared
    assert 0 < len(want) and any(c >= 3 for c in per) and any(c == 0 for c in per) and len(want) != len(s.all_f)
    assert len(want) >= sum(c for i, c in enumerate(s.counts) if i % 8 != 7)      # (every planted indicator of the UTF-8 lines at least)
    assert any(f["s"].encode().startswith((b"http", b"1", b"2")) and c for f, c in zip(s.all_f, per))
    texts = {f["s"] for f in want}
    assert any(t.startswith("https://") for t in texts) and any("@" in t for t in texts) and any(re.fullmatch(r"[0-9.]+", t) for t in texts)
    print(len(want), "matches in", len(s.all_f), "findings; by Mission:", {m: sum(f["mission_id"] == m for f in want) for m in {f["mission_id"] for f in s.all_f}})
    xs = s.sc.extract_set(pats)
    ext = s.res.extract_device(xs)
    check_extraction(s.sc, s.src, ext, want, per, s.ms, prints=True)
    ext.free(); xs.free()
    # the fold
    up = [URL.upper().replace(b"S?", b"s?"), MAIL.upper()]
    w2, _ = extract_and_check(s, up, nocase=True)
    assert len(w2) > 0 and expected(s.all_f, up)[0] == []


@pytest.fixture(scope="module")
def case_a():
    ms, data, _ = case("A")
    ref = sx.Scanner(ms, device=0)
    host = ref.scan(data, file_id=1)
    all_f = host.findings()
    host.free(); ref.close()
    assert len(all_f) > 1000
    return dict(ms=ms, data=data, all_f=all_f)


SHAPES = [([rb"[0-9]{3}\.[0-9]"], False), ([rb"(=|:)[a-z]*(=|:)"], False), ([rb"[a-h]{2}$", rb"^x[0-9]"], True)]


def test_case_a_with_a_handful_of_shapes(case_a):
    a = case_a
    s = Source(a["ms"], a["data"], all_f=a["all_f"])
    try:
        for k, (pats, nocase) in enumerate(SHAPES):
            want, per = extract_and_check(s, pats, nocase, prints=k == 0)
            print(pats, len(want), "matches in", len(a["all_f"]), "findings")
            assert 0 < len(want) and len(want) != len(a["all_f"])
    finally:
        s.close()


def test_one_mission_sparse_unpacked_segment():
    """the lane-per-region replay's segment: sx_finding records, strings where the writer put them"""
    data = synth(random.Random(78), 4_000_000, 1 / 400)
    s = Source(rc.missions(encodings=["utf-8"], chars_min="10"), data, device_replay=True)
    try:
        assert len(s.all_f) >= 100 and all(not seg[4] for seg in s.src)
        pats = [rb"[a-z]{2,5}", rb"[0-9]+", rb"^/usr"]      # (the planted words: a sentence has many, a run of capitals or of Armenian none)
        want, per = extract_and_check(s, pats)
        assert 0 < len(want) and any(c >= 2 for c in per) and any(c == 0 for c in per)
    finally:
        s.close()


def test_composition_with_selection_tally_and_print(planted_source):
    s = planted_source
    sc, res, ms, all_f = s.sc, s.res, s.ms, s.all_f
    xs_all, xs_mail, xs_host = sc.extract_set([URL, MAIL, QUAD]), sc.extract_set([MAIL]), sc.extract_set([rb"@[a-z-]+"])
    # the extraction of a selection
    sel = res.select_device(b"charlie")
    sel_f = [f for f in all_f if "charlie" in f["s"]]
    want, per = expected(sel_f, [MAIL])
    assert 0 < len(want) and 0 < len(sel_f) < len(all_f)
    ext = sel.extract_device(xs_mail)
    check_extraction(sc, sel.device_segments(), ext, want, per, ms)
    sel.free(); ext.free()
    # a selection, a tally and a print of an extraction
    want, per = expected(all_f, [URL, MAIL, QUAD])
    ext = res.extract_device(xs_all)
    src_ptrs = pointers(ext)
    keys = [b"example.com", b"https", b"golf", b"zzz"]
    ts = sc.tally_set(keys)
    assert ext.tally_device(ts) == len(want)
    hits, _ = ts.read()
    by_python = [sum(f["s"].encode().count(k) for f in want) for k in keys]      # (no key overlaps itself)
    assert hits == by_python and hits[0] > 0 and hits[1] > 0 and hits[3] == 0
    ts.free()
    only = ext.select_device(b"https://")
    want_only = [f for f in want if "https://" in f["s"]]
    assert 0 < len(want_only) < len(want) and downloaded(sc, only) == want_only
    p, n = ext.printed_device(n_inputs=1, radix="x")
    text = sc.download(C.c_void_p(p), n)
    assert pointers(ext) == src_ptrs
    assert text == ext.printed(n_inputs=1, radix="x") == printed_by_python(want, ms, "x", False)      # (the host accessor fetches the extraction)
    only.free(); ext.free()
    # an extraction of an extraction, with a narrower pattern
    ext = res.extract_device(xs_all)
    again = ext.extract_device(xs_host)
    w2, p2 = expected(want, [rb"@[a-z-]+"])
    assert 0 < len(w2) < len(want)
    check_extraction(sc, ext.device_segments(), again, w2, p2, ms)
    ext.free(); again.free()
    for x in (xs_all, xs_mail, xs_host):
        x.free()


def test_results_and_lifetime(planted_source):
    s = planted_source
    sc, res, all_f = s.sc, s.res, s.all_f
    xs, none = sc.extract_set([QUAD]), sc.extract_set([rb"\x02never"])
    before = pointers(res)
    empty = res.extract_device(none)                  # counts as a selection
    assert len(empty) == 0 and empty.device_segments() == [] and empty.segments() == [] and empty.findings() == []
    assert code_of(lambda: empty.extract_device(xs)) == sx.SX_E_STATE        # the empty result is in host memory
    want, per = expected(all_f, [QUAD])
    e1 = res.extract_device(xs)
    assert pointers(res) == before                    # the source: read, never moved
    assert res.findings() == all_f                    # ... and its host accessors work as before (they fetch it)
    res2 = sc.scan(s.data, file_id=1)                 # a scan in between does not invalidate an extraction
    assert downloaded(sc, e1) == want
    s1 = res2.select_device(b"golf")                  # one selection later: still there
    assert downloaded(sc, e1) == want
    assert code_of(lambda: e1.extract_device(xs)) == sx.SX_E_STATE           # its block is the one this call would write; a refused call does not count
    assert downloaded(sc, e1) == want
    s2 = res2.extract_device(xs)                      # the second selection after it takes its block
    assert code_of(e1.device_segments) == sx.SX_E_STATE and code_of(lambda: e1.extract_device(xs)) == sx.SX_E_STATE
    assert len(s2) > 0
    for r in (empty, e1, s1, s2):
        r.free()
    # the planted source goes on with the new scan's result
    res.free()
    s.res, s.src, s.before = res2, res2.device_segments(), pointers(res2)
    xs.free(); none.free()


def test_errors_are_codes():
    ms, data, _ = case("D")
    host_sc = sx.Scanner(ms, device=0)                # results in host memory
    host = host_sc.scan(data, file_id=1)
    xs = host_sc.extract_set([b"[a-z]+"])
    assert len(host) > 0 and code_of(lambda: host.extract_device(xs)) == sx.SX_E_STATE
    rs = host_sc.regex_set([b"[a-z]+"])
    with pytest.raises(TypeError):
        host.extract_device(rs)
    with pytest.raises(TypeError):
        host.select_device(xs)
    with pytest.raises(TypeError):
        host.extract_device([b"[a-z]+"])
    with pytest.raises(sx.SxError) as e:
        host_sc.extract_set([b"ok", rb"a\b"])
    assert e.value.code == sx.SX_E_INVALID and "pattern 1, offset 1" in str(e.value)
    assert code_of(lambda: host_sc.extract_set([])) == sx.SX_E_INVALID
    # a set from another context on the same device works
    other = sx.Scanner(ms, device=0, result_on_device=True)
    theirs = other.scan(data, file_id=1)
    want, per = expected(host.findings(), [b"[a-z]+"])
    ext = theirs.extract_device(xs)
    assert 0 < len(want) and downloaded(other, ext) == want
    ext.free(); theirs.free(); other.close()
    host.free(); host_sc.close()
    # a host-only context
    cpu = sx.Scanner(ms, device=sx.SX_HOST_ONLY)
    assert code_of(lambda: cpu.extract_set([b"a"])) == sx.SX_E_STATE
    assert code_of(lambda: cpu.extract_set([rb"a\b"])) == sx.SX_E_INVALID      # (the patterns are judged first)
    cpu.close()
    assert xs.info()["n_patterns"] == 1               # the set outlives its Scanner
    xs.free(); rs.free()
    assert code_of(xs.info) == sx.SX_E_INVALID
