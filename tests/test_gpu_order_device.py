"""sx_result_order_device (include/stringsext_amd.h): the findings of a result that lies in HBM in sorted order — by string, by string
under the ASCII fold, by a field of a label word —, ascending and descending, filtered by a label pick, cut at a limit, on the device
(stringsext_amd/csrc/sx_order_dev.hip).  No expected value comes from the code under test: the strings are the oracle's
(tests/result_plant.py expected()) or the lines the test planted, the order is Python's sorted() over them (tests/test_order_core.py
model(), which also gives the numbers of sx_order_info), the label words are models over the same strings, and the records are the
source's own, downloaded and expanded by the test.

The sources are small: tests/result_plant.py prefix(k) under one Mission on the wave path (packed records) and on the lane-per-region
replay (unpacked), under two Missions (every line found twice, merged, packed), and Cyrillic lines under one UTF-8 Mission; the
counts that take part are 0, 1, 2, 63, 64, 65, 127, 128, 129 and 513, and one case has one record more than a trip of the kernels'
grid."""
import collections

import numpy as np
import pytest

import refconfig as rc
import result_plant as rp
import stringsext_amd as sx
from test_gpu_result_on_device_multi import F16, F32, expanded
from test_gpu_result_strides import constant
from test_gpu_select_device import downloaded
from test_gpu_select_set_device import code_of
from test_order_core import fold, model, picked

pytestmark = pytest.mark.gpu

FIRST, REPEATED, SHIFT = sx.SX_DISTINCT_FIRST, sx.SX_DISTINCT_REPEATED, sx.SX_DISTINCT_COUNT_SHIFT
QUIET, TWO_WINDOWS = b"\x80", 2 * 4096      # a byte in which neither `-e ascii` nor `-e utf-8` reads a character; the wave path takes buffers of two windows or more
NO_BIT = 1 << 62                            # a bit no label word of these tests has
SPECS = [("one", k) for k in (1, 2, 63, 64, 65, 127, 128, 129, 513)] + [("replay", 65), ("replay", 513), ("two", 32), ("two", 64), ("cyrillic", 129)]


def cyrillic_lines(k):
    """k lines of Cyrillic and ASCII words: classes of equal lines, lines that are prefixes of others, lines that part behind 8 and 16 bytes"""
    words = ["привет", "мир", "строка", "Привет", "поиск", "ёж", "data", "Zeta", "zeta"]
    out = []
    for i in range(k):
        a, b, c = words[i % 9], words[i * 7 % 9], words[i * 5 % 8]
        out.append(("%s %s %s" % (a, b, c) if i % 3 else "%s %s" % (a, b)).encode("utf-8") + (b" %d" % (i % 11) if i % 4 == 1 else b""))
    return out


@pytest.fixture(scope="module")
def scanners():
    ms1, ms2, ms8 = rp.ms1(), rp.ms2(), rc.missions(encodings=["utf-8"], chars_min="4")
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SX_WAVE_REPLAY", "1")                    # (a context keeps the switches it was created under)
        out["one"] = (ms1, sx.Scanner(ms1, device=0, result_on_device=True))
        out["cyrillic"] = (ms8, sx.Scanner(ms8, device=0, result_on_device=True))
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SX_WAVE_REPLAY", "0")
        out["replay"] = (ms1, sx.Scanner(ms1, device=0, device_replay=True, result_on_device=True))
    out["two"] = (ms2, sx.Scanner(ms2, device=0, result_on_device=True))
    yield out
    for _, sc in out.values():
        sc.close()


def fetched(sc, res):
    """a source's findings as they lie on the device, expanded by the test (no layout is assumed: a single Mission's strings lie where
    the writer put them)"""
    out = []
    for fp, n, ap, alen, packed, info in res.device_segments():
        recs = np.frombuffer(sc.download(fp, n * (16 if packed else 32)), dtype=F16 if packed else F32)
        out += expanded(recs, sc.download(ap, alen) if alen else b"", packed, info)
    return out


class Case:
    """a result on the device, its findings as the test downloaded them, and their strings, which are the oracle's"""

    def __init__(self, name, sc, res, ms, strs):
        self.name, self.sc, self.res, self.ms = name, sc, res, ms
        self.src_f = fetched(sc, res)
        self.strs = [f["s"].encode("utf-8") for f in self.src_f]
        assert self.strs == strs, name
        self.n = len(strs)


def scan_case(name, ms, sc, data, count=None):
    rows = rp.expected(ms, data)
    sc.reset()                                              # (every buffer is a stream of its own)
    res = sc.scan(data, file_id=1)
    segs = res.device_segments()
    assert len(res) == rows.n and (count is None or rows.n == count), (name, len(res), rows.n, count)
    assert all(g[0] and g[2] for g in segs), name
    return Case(name, sc, res, ms, rows.strs)


@pytest.fixture(scope="module", params=SPECS, ids=["%s-%d" % spec for spec in SPECS])
def source(request, scanners):
    kind, k = request.param
    ms, sc = scanners[kind]
    data = b"\n".join(cyrillic_lines(k)) + b"\n" if kind == "cyrillic" else rp.prefix(k)
    if kind in ("one", "cyrillic"):
        data += QUIET * max(0, TWO_WINDOWS - len(data))
    c = scan_case("%s-%d" % (kind, k), ms, sc, data, k * len(ms))
    assert [g[4] for g in c.res.device_segments()] == [kind != "replay"]      # (the lane-per-region replay's records are sx_finding)
    yield c
    c.res.free()


def distinct_words(strs):
    words, _, _, _ = rp.distinct_model(strs, FIRST, REPEATED, SHIFT)
    return [int(w) for w in words]


def labels_of(c, res, want):
    """distinct_device()'s Labels of `res`, which have to be the model's words"""
    lab = res.distinct_device()
    assert [w for seg in lab.download() for w in seg] == want, c.name
    return lab


def counted(c):
    """(a counted seen set that held this result and then its findings with SUBSTRING, the model of its count words per finding)"""
    ss = c.sc.seen_set(c.n + 8, sum(len(s) for s in c.strs) + 16 * c.n + 64, counted=True)
    c.res.seen_device(ss).free()
    sub = [s for s in c.strs if rp.SUBSTRING in s]
    if sub:
        sel = c.res.select_device(rp.SUBSTRING)
        sel.seen_device(ss).free()
        sel.free()
    once, again = collections.Counter(c.strs), collections.Counter(sub)
    return ss, [(1 + (s in again)) << sx.SX_SEEN_RESULTS_SHIFT | (once[s] + again[s]) << sx.SX_SEEN_FINDINGS_SHIFT for s in c.strs]


def check_order(c, res, src_f, strs, key, labels, words, descending, any_, limit, prints=True):
    """one call against the model; returns the ordered findings"""
    part = [i for i in range(len(strs)) if not any_ or picked(words[i], any_, 0, 0)]
    if key in ("string", "nocase"):
        keys, kw = [fold(strs[i]) if key == "nocase" else strs[i] for i in part], dict(by="string", ignore_case=key == "nocase")
    else:
        shift = SHIFT if key == "count" else sx.SX_SEEN_RESULTS_SHIFT
        keys, kw = [words[i] >> shift & 0xFFFFFFFF for i in part], dict(by="field", shift=shift, bits=32)
    order, info = model(keys, descending, limit, key in ("string", "nocase"))
    out = res.order_device(labels=labels if (any_ or kw["by"] == "field") else None, descending=descending, any=any_, limit=limit, **kw)
    what = (c.name, key, descending, any_, limit)
    assert out.order_info == info, (what, out.order_info, info)
    want = [src_f[part[i]] for i in order[:info["kept"]]]
    segs = out.device_segments()
    assert len(out) == len(want) and [(g[1], g[4]) for g in segs] == ([(len(want), False)] if want else []), what
    got = downloaded(c.sc, out) if want else []
    assert got == want, (what, next(((p, a, b) for p, (a, b) in enumerate(zip(got, want)) if a != b), None))
    if want and prints:
        p, n = out.printed_device(radix="x")
        text = c.sc.download(p, n)
        assert text == out.printed(radix="x") and all(f["s"].encode() in text for f in want[:3]), what      # (printed() last: the host accessors fetch the result)
    out.free()
    return want


def test_every_key_direction_filter_and_limit(source):
    c = source
    dwords = distinct_words(c.strs)
    d = labels_of(c, c.res, dwords)
    ss, cwords = counted(c)
    counts = c.res.seen_counts_device(ss)
    assert [w for seg in counts.download() for w in seg] == cwords, c.name
    try:
        for key, labels, words in (("string", d, dwords), ("nocase", d, dwords), ("count", d, dwords), ("seen", counts, cwords)):
            for descending in (False, True):
                for any_ in (0, FIRST):
                    for limit in (0, 20):
                        check_order(c, c.res, c.src_f, c.strs, key, labels, words, descending, any_, limit, prints=limit == 0 or key == "string")
        # nothing takes part: a result without segments, and the call counts like a selection that selects nothing
        assert check_order(c, c.res, c.src_f, c.strs, "string", d, dwords, False, NO_BIT, 0) == []
        if c.n >= 63:
            firsts = sum(1 for w in dwords if w & FIRST)
            assert 0 < firsts < c.n and any(w >> SHIFT >= 3 for w in dwords)      # the filter drops something, and a class of three or more is tied
    finally:
        d.free(); counts.free(); ss.free()


def test_an_order_of_an_order_is_the_identity_and_feeds_the_family(scanners):
    ms, sc = scanners["one"]
    data = rp.prefix(513)
    c = scan_case("chain", ms, sc, data + QUIET * max(0, TWO_WINDOWS - len(data)), 513)
    try:
        for kw in (dict(), dict(descending=True), dict(ignore_case=True)):
            first = c.res.order_device(**kw)
            want = downloaded(sc, first)
            key = (lambda f: fold(f["s"].encode())) if kw.get("ignore_case") else (lambda f: f["s"].encode())
            assert want == sorted(c.src_f, key=key, reverse=bool(kw.get("descending")))
            again = first.order_device(**kw)
            assert downloaded(sc, again) == want, kw
            again.free(); first.free()
        # an ORDER as the source of a selection, a distinct call and a tally
        o = c.res.order_device()
        sorted_f = sorted(c.src_f, key=lambda f: f["s"].encode())
        sorted_s = [f["s"].encode() for f in sorted_f]
        sel = o.select_device(rp.SUBSTRING)
        assert downloaded(sc, sel) == [f for f in sorted_f if rp.SUBSTRING in f["s"].encode()] and 0 < len(sel) < len(o)
        sel.free()
        lab = labels_of(c, o, distinct_words(sorted_s))
        assert lab.info["distinct"] == len(set(c.strs))
        lab.free()
        ts = sc.tally_set([rp.SUBSTRING, b"key="])
        assert o.tally_device(ts) == 513
        assert ts.read()[0] == [sum(s.count(p) for s in c.strs) for p in (rp.SUBSTRING, b"key=")]
        ts.free(); o.free()
        # sort -u: distinct, then the firsts in order
        d = c.res.distinct_device()
        u = c.res.order_device(labels=d, any=FIRST)
        assert [f["s"].encode() for f in downloaded(sc, u)] == sorted(set(c.strs)) and u.order_info["tied"] == 0
        u.free(); d.free()
    finally:
        c.res.free()


def test_a_source_of_several_packed_segments():
    """the merged result of two Missions cut into parts: equal strings of different segments come out in segment order"""
    ms = rp.ms2()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SX_MERGE_PART_FINDINGS", "7000")
        mp.setenv("SX_MERGE_PART_MIB", "1")
        sc = sx.Scanner(ms, device=0, result_on_device=True)
    try:
        c = scan_case("parts", ms, sc, rp.buffer(12000))
        segs = c.res.device_segments()
        assert len(segs) >= 3 and all(g[4] for g in segs)
        seg_of = [k for k, g in enumerate(segs) for _ in range(g[1])]
        first_seg = {}
        assert sum(first_seg.setdefault(s, k) != k for k, s in zip(seg_of, c.strs)) > 0      # a class with members in two segments
        dwords = distinct_words(c.strs)
        d = labels_of(c, c.res, dwords)
        for key, descending, any_, limit in (("string", False, 0, 0), ("nocase", True, 0, 0), ("string", False, FIRST, 0), ("count", True, FIRST, 20), ("count", False, 0, 0)):
            want = check_order(c, c.res, c.src_f, c.strs, key, d, dwords, descending, any_, limit, prints=key == "count")
        assert len(want) == c.n
        top = check_order(c, c.res, c.src_f, c.strs, "count", d, dwords, True, FIRST, 20)      # uniq -c | sort -rn | head -20
        assert top[0]["s"].encode() == rp.DOMINANT and len(top) == 20
        d.free(); c.res.free()
    finally:
        sc.close()


def test_one_record_more_than_a_trip_of_the_grid(scanners):
    """R + 1 lines of 16 bytes that share their first 8 and part in their last 8: round 0 decides nothing, round 1 everything, and
    every kernel's second trip holds one record"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    r = cus * constant("kOrderGroupsPerCu") * constant("kRowsWaves") * constant("kSelectRecs")
    n = r + 1
    k = np.arange(n, dtype=np.uint64)
    number = k * np.uint64(2654435761) % np.uint64(99999989)           # (a prime: one to one below it; 8 digits)
    assert n < 99999989 and len(np.unique(number)) == n
    lines = np.char.add(b"trip 000", np.char.zfill(number.astype("S8"), 8))
    data = b"\n".join(lines.tolist()) + b"\n"
    assert len(data) == 17 * n
    ms, sc = scanners["one"]
    sc.reset()
    res = sc.scan(data, file_id=1)
    try:
        segs = res.device_segments()
        assert len(res) == n and len(segs) == 1 and segs[0][0] and segs[0][4], [(g[0], g[1], g[4]) for g in segs]      # one packed segment: line k is finding k
        out = res.order_device()
        assert out.order_info == dict(findings=n, kept=n, rounds=2, tied=0, max_depth=1)
        (fp, m, ap, alen, packed, _), = out.device_segments()
        assert (m, alen, packed) == (n, 16 * n, False)
        recs = np.frombuffer(sc.download(fp, 32 * n), dtype=F32)
        want = np.argsort(number, kind="stable").astype(np.uint64)      # (the lines differ in their numbers alone, zero-padded: their order is the numbers')
        src = np.frombuffer(sc.download(segs[0][0], 16 * n), dtype=F16)      # (a position is the finding's window, not its line: the source's own, permuted)
        assert np.all(src["str_len"] == 16) and np.all(np.diff(src["position"].astype(np.int64)) >= 0)
        assert np.array_equal(recs["position"], src["position"][want.astype(np.int64)]) and np.array_equal(recs["mission_id"], src["mission_id"][want.astype(np.int64)])
        assert np.array_equal(recs["str_off"], np.arange(n, dtype=np.uint32) * np.uint32(16))
        assert np.all(recs["str_len"] == 16) and np.all(recs["file_id"] == 1)
        assert sc.download(ap, alen) == b"".join(lines[want.astype(np.int64)].tolist())
        # the last line of the order, and descending with a limit: the largest numbers first
        tail = res.order_device(descending=True, limit=3)
        assert [f["s"].encode() for f in downloaded(sc, tail)] == lines[want.astype(np.int64)][::-1][:3].tolist()
        tail.free(); out.free()
    finally:
        res.free()


def test_the_blocks_take_turns_and_a_refused_call_takes_none(scanners):
    ms, sc = scanners["two"]
    c = scan_case("turns", ms, sc, rp.prefix(40), 80)
    try:
        d = c.res.distinct_device()
        one, two = c.res.order_device(), c.res.order_device(descending=True)
        # the source of a third call lies in the block that call would write
        assert code_of(one.order_device) == sx.SX_E_STATE and "two calls ago" in sx.lib().sx_last_error(sc.h).decode()
        assert downloaded(sc, one) == sorted(c.src_f, key=lambda f: f["s"].encode())           # refused: nothing was written, no turn taken
        three = two.order_device()                                                              # the third turn: `one`'s block
        assert code_of(lambda: one.printed_device()) == sx.SX_E_STATE
        # calls that are SX_E_INVALID take no turn: the next call still writes `two`'s block, not `three`'s
        assert code_of(lambda: three.order_device(by="field")) == sx.SX_E_INVALID              # no labels for the field
        assert code_of(lambda: three.order_device(labels=d, any=FIRST)) == sx.SX_E_INVALID     # labels of another result
        assert "not made from this result" in sx.lib().sx_last_error(sc.h).decode()
        assert code_of(lambda: three.order_device(by="field", labels=d, ignore_case=True)) == sx.SX_E_INVALID
        four = three.order_device(descending=True)
        assert downloaded(sc, four) == sorted(c.src_f, key=lambda f: f["s"].encode(), reverse=True)
        assert code_of(lambda: two.printed_device()) == sx.SX_E_STATE
        for x in (one, two, three, four, d):
            x.free()
        # a source that a later scan has overwritten
        stale = c.res
        fresh = sc.scan(rp.prefix(40), file_id=1)
        assert code_of(stale.order_device) == sx.SX_E_STATE
        fresh.free()
    finally:
        c.res.free()
