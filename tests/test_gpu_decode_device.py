"""sx_result_decode_device (Result.decode_device): the strings of a result that lies in HBM read as base64, hex or percent escapes on
the device, and what the other operations make of the decoded bytes — over the lines of tests/decode_plant.py.

The sources, as in tests/test_gpu_fold_device.py
    wave k     one UTF-8 Mission on the wave path, packed records, ONE segment of k findings: k = 1, 63, 64, 65, 129 — around a
               wavefront's 64 records and past two — and R + 1, R = CUs x kRowsGroupsPerCu x kRowsWaves x 64 read from the sources as
               tests/test_gpu_result_strides.py reads them: the one record of the kernels' second trip
    lane k     the same Mission on the lane-per-region replay, the lines behind the buffer's first window: unpacked records,
               strings where the writer put them; the small k
    merged     two Missions, `-e ascii -e utf-8`, under SX_MERGE_PART_FINDINGS=1024: packed, several segments, strings back to back
    long       decode_plant.long_lines() at `-q 1024`, merged and packed; limit: decode_plant.limit_lines() at `-q 16000`

Every expected value is the oracle's text (result_plant.expected()) and decode_plant.decode() — the rule in Python, which takes its
bytes from base64, binascii, urllib.parse and codecs — over its strings; no value comes from a product Scanner."""
import ctypes as C
import re

import numpy as np
import pytest

import decode_plant as dp
import fold_plant as fp
import long_plant as lp
import measure_plant as mp
import result_plant as rp
import stringsext_amd as sx
from test_gpu_fold_device import QUIET, TWO_WINDOWS, raw_records
from test_gpu_result_strides import check_records, picked, printed_on_device, same, trip_sizes, words_of
from test_gpu_select_device import info_tuple

pytestmark = pytest.mark.gpu

FIRST, REPEATED, SHIFT = sx.SX_DISTINCT_FIRST, sx.SX_DISTINCT_REPEATED, sx.SX_DISTINCT_COUNT_SHIFT
SMALL = (1, 63, 64, 65, 129)
MERGED_LINES = 3000
PARTS = (("SX_MERGE_PART_FINDINGS", "1024"), ("SX_MERGE_PART_MIB", "1"))
KINDS = ["base64", "hex", "percent"]
ALL = [(kind, utf16le) for kind in KINDS for utf16le in (False, True)]


class Src:
    def __init__(self, name, sc, res, rows):
        self.name, self.sc, self.res, self.rows = name, sc, res, rows

    def close(self):
        self.res.free(); self.sc.close()


def make(name, kind, ms, data, env=()):
    """kind: `wave` (packed, one segment), `lane` (the lane-per-region replay: unpacked, the lines behind the buffer's first window) or
    `merged` (several Missions: packed, strings back to back)"""
    kw = {}
    if kind == "lane":      # (the buffer's first window is replayed by the host: the lines lie behind it, where the device writes them)
        data, env, kw = QUIET * 4096 + data, (("SX_WAVE_REPLAY", "0"),), dict(device_replay=True)
    elif kind == "wave":
        env = (("SX_WAVE_REPLAY", "1"),)
    if kind != "merged":
        data += QUIET * max(0, TWO_WINDOWS - len(data))
    rows = rp.expected(ms, data)
    with pytest.MonkeyPatch.context() as patch:
        for key, v in env:
            patch.setenv(key, v)
        sc = sx.Scanner(ms, device=0, result_on_device=True, **kw)      # (a context keeps the switches it was created under)
    res = sc.scan(data, file_id=1)
    segs = res.device_segments()
    assert len(res) == rows.n and all(g[0] for g in segs), (name, len(res), rows.n)
    assert [g[4] for g in segs] == [kind != "lane"] * len(segs), (name, [g[4] for g in segs])
    assert (len(ms) > 1) == (kind == "merged") and (kind != "wave" or len(segs) == 1)
    return Src(name, sc, res, rows)


def planted(kind, k):
    if kind == "merged":
        s = make("merged %d" % k, kind, fp.ms2(), dp.buffer(k), PARTS)
        assert len(s.res.device_segments()) >= 3 and s.rows.n == 2 * k
    else:
        s = make("%s %d" % (kind, k), kind, fp.ms1(), dp.buffer(k))
        assert s.rows.strs == dp.lines(k)
    return s


MAKERS = {
    "long": lambda: make("long", "merged", fp.msl(), lp.buffer(dp.long_lines())),
    "limit": lambda: make("limit", "merged", lp.limit_ms(), lp.buffer(dp.limit_lines())),
    "plain": lambda: make("plain", "wave", fp.ms1(), rp.buffer(129)),      # result_plant's lines: nothing in them is hex or an escape
}


@pytest.fixture(scope="module")
def sources():
    made = {}

    def get(kind, k=None):
        if (kind, k) not in made:
            made[kind, k] = MAKERS[kind]() if k is None else planted(kind, k)
        return made[kind, k]
    yield get
    for s in made.values():
        s.close()


def flags_of(utf16le):
    return dp.UTF16LE if utf16le else 0


def replaced_text(rows, strs):
    """the oracle's text with every string replaced"""
    raw = [r[:len(r) - len(s)] + o for r, s, o in zip(rows.raw, rows.strs, strs)]
    return rp.OUTPUT_BOM + b"".join(b"\n" + r for r in raw) + b"\n"


def check_decode(s, res, d, kind, utf16le, rows=None, printed=True):
    """`d`, decoded from `res` whose rows are `rows`: segment for segment the source's shape, record for record the source's fields,
    the strings the rule's over the oracle's, back to back; the words, bound to the source; the info; the text.  Returns (the rows of
    d, the words)"""
    rows = rows or s.rows
    what = "%s: %s%s" % (s.name, kind, " utf16le" if utf16le else "")
    outs = dp.decoded(dp.KINDS[kind], flags_of(utf16le), rows.strs)
    drows = rows.take(np.arange(rows.n), strs=[o for o, _ in outs])
    want_words = np.array([w for _, w in outs], dtype=np.uint64)
    src, got = res.device_segments(), d.device_segments()
    assert [(g[1], g[4], info_tuple(g[5])) for g in got] == [(g[1], g[4], info_tuple(g[5])) for g in src], what
    for g in got:
        assert g[0] % 256 == 0 and g[2] == g[0] + g[1] * (16 if g[4] else 32)                      # [records][strings], 256-byte aligned
    assert all(len(o) > 0 for o in drows.strs)                                                      # no empty string arises
    check_records(s.sc, d, drows, True, what)
    for (packed, a), (_, b) in zip(raw_records(s.sc, res), raw_records(s.sc, d)):
        keep = np.ones(a.shape[1], dtype=bool)
        keep[8:14 if packed else 16] = False                                                        # str_off and str_len
        assert np.array_equal(a[:, keep], b[:, keep]), what                                         # every other byte of every record
    same(words_of(s.sc, d.decode_words, res), want_words, what + ": words", rows.strs)
    want = dp.info(rows.strs, outs)
    assert d.decode_info == want, (what, d.decode_info, want)
    if printed and rows.raw is not None:
        got_text, want_text = printed_on_device(s.sc, d), replaced_text(rows, drows.strs)
        assert len(got_text) == len(want_text) and got_text == want_text, (what, len(got_text), len(want_text))
    return drows, want_words


@pytest.mark.parametrize("kind,utf16le", ALL)
@pytest.mark.parametrize("k", SMALL)
@pytest.mark.parametrize("path", ["wave", "lane"])
def test_one_mission_around_a_wavefront(sources, path, k, kind, utf16le):
    s = sources(path, k)
    d = s.res.decode_device(kind, utf16le=utf16le)
    check_decode(s, s.res, d, kind, utf16le)
    assert k < 63 or 0 < d.decode_info["decoded"] < k
    d.decode_words.free(); d.free()


@pytest.mark.parametrize("kind,utf16le", ALL)
def test_merged_missions_in_several_segments_and_the_words_both_ways(sources, kind, utf16le):
    s = sources("merged", MERGED_LINES)
    d = s.res.decode_device(kind, utf16le=utf16le)
    drows, words = check_decode(s, s.res, d, kind, utf16le)
    info = d.decode_info
    assert 0 < info["text"] < info["decoded"] < info["findings"] and 0 < info["wide"] and info["bytes_in"] != info["bytes_out"]
    # the words, bound to the decoded result: what decodes to text, selected there ...
    bound = d.decode_words.rebind(d)
    same(words_of(s.sc, bound, d), words, s.name + ": the rebound words")
    for res, labels in ((s.res, bound), (d, d.decode_words)):      # (the new labels are the decoded result's, the old ones the source's)
        with pytest.raises(sx.SxError) as e:
            res.select_device(labels, all=sx.SX_DECODE_OK)
        assert e.value.code == sx.SX_E_INVALID
    mask = picked(words, 0, sx.SX_DECODE_OK | sx.SX_DECODE_TEXT, 0)
    sel = d.select_device(bound, all=sx.SX_DECODE_OK | sx.SX_DECODE_TEXT)
    check_records(s.sc, sel, drows.take(np.nonzero(mask)[0], strs=[x for x, m in zip(drows.strs, mask) if m]), True, s.name + ": decoded text")
    sel.free(); bound.free()
    # ... and the way back: labels of the decoded bytes, bound to the source, select the ENCODED originals
    patterns = [rb"[Nn]et", rb"\x00", rb"^[a-z]+:"]
    rx = [re.compile(p) for p in patterns]
    lab_words = np.array([sum(1 << p for p, r in enumerate(rx) if r.search(x)) for x in drows.strs], dtype=np.uint64)
    ls = s.sc.label_set(patterns)
    lab = d.label_device(ls)
    same(words_of(s.sc, lab, d), lab_words, s.name + ": labels of the decoded bytes", drows.strs)
    back = lab.rebind(s.res)
    hit = picked(lab_words, 0b111, 0, 0)
    assert 0 < hit.sum() < s.rows.n
    sel = s.res.select_device(back, any=0b111)
    check_records(s.sc, sel, s.rows.take(hit), True, s.name + ": the encoded originals")
    sel.free(); back.free(); lab.free(); ls.free(); d.decode_words.free(); d.free()


@pytest.mark.parametrize("kind,utf16le", ALL)
def test_one_record_in_the_second_trip(sources, kind, utf16le):
    r, _ = trip_sizes()
    s = sources("wave", r + 1)
    d = s.res.decode_device(kind, utf16le=utf16le)
    check_decode(s, s.res, d, kind, utf16le)
    assert d.decode_info["findings"] == r + 1 and 0 < d.decode_info["decoded"] < r
    d.decode_words.free(); d.free()


@pytest.fixture(scope="module")
def merged(sources):
    return sources("merged", MERGED_LINES)


def test_measure_on_decoded_bytes_sets_the_control_bit(merged):
    s = merged
    for kind in KINDS:
        d = s.res.decode_device(kind)
        strs = [o for o, _ in dp.decoded(dp.KINDS[kind], 0, s.rows.strs)]
        want = np.array([mp.measure(x) for x in strs], dtype=np.uint64)
        control = want & np.uint64(sx.SX_MEASURE_CONTROL) != 0
        assert 0 < control.sum() < s.rows.n and not any(mp.measure(x) & mp.CONTROL for x in s.rows.strs)      # only decoding brings such bytes
        m = d.measure_device()
        same(words_of(s.sc, m, d), want, "%s: measure words of %s" % (s.name, kind), strs)
        assert m.info == mp.info(strs)
        m.free(); d.decode_words.free(); d.free()


def test_label_select_distinct_and_fold_on_decoded_bytes_that_are_no_text(merged):
    s = merged
    d = s.res.decode_device("base64")
    outs = dp.decoded(dp.BASE64, 0, s.rows.strs)
    strs = [o for o, _ in outs]
    drows = s.rows.take(np.arange(s.rows.n), strs=strs)
    assert sum(1 for x in strs if {0x00, 0x0A, 0xFF} <= set(x)) >= 4
    # labels: a NUL, an 0xFF, a line feed between two bytes, four letters
    patterns = [rb"\x00", rb"\xff", rb"[^\n]\n[^\n]", rb"[A-Za-z]{4}"]
    rx = [re.compile(p) for p in patterns]
    want = np.array([sum(1 << p for p, r in enumerate(rx) if r.search(x)) for x in strs], dtype=np.uint64)
    assert all(0 < (want >> np.uint64(p) & np.uint64(1)).sum() < s.rows.n for p in range(4))
    ls = s.sc.label_set(patterns)
    lab = d.label_device(ls)
    same(words_of(s.sc, lab, d), want, s.name + ": labels of decoded bytes", strs)
    lab.free(); ls.free()
    # sort -u of the decoded bytes
    words, info, _, _ = rp.distinct_model(strs, FIRST, REPEATED, SHIFT)
    lab = d.distinct_device()
    same(words_of(s.sc, lab, d), words, s.name + ": distinct words of decoded bytes", strs)
    assert {k: lab.info[k] for k in ("findings", "distinct", "repeated")} == info
    lab.free()
    # the fold of the decoded bytes: ill-formed UTF-8 is copied (one selection after d: d stays valid)
    folded = [fp.fold(x) for x in strs]
    assert any(f != x for f, x in zip(folded, strs))
    f = d.fold_device()
    check_records(s.sc, f, drows.take(np.arange(drows.n), strs=folded), True, s.name + ": the fold of decoded bytes")
    f.free(); d.decode_words.free(); d.free()
    # a substring of bytes that no scan finds in a string
    d = s.res.decode_device("base64")
    needle = b"\x00\x0a\xff"
    mask = np.array([needle in x for x in strs], dtype=bool)
    assert 0 < mask.sum() < s.rows.n
    sel = d.select_device(needle)
    check_records(s.sc, sel, drows.take(np.nonzero(mask)[0], strs=[x for x, m in zip(strs, mask) if m]), True, s.name + ": selected by bytes")
    sel.free(); d.decode_words.free(); d.free()


CUT_PATTERNS = [rb"[a-z0-9]*%[0-9]", rb"[0-9][a-z0-9]+"]      # an escape cut behind its first digit: `x%4` `1y`, back to back in the arena


@pytest.mark.parametrize("kind,utf16le", [("percent", False), ("percent", True), ("hex", False), ("base64", True)])
def test_an_extraction_decoded_no_decoder_reads_past_its_record(merged, kind, utf16le):
    s = merged
    # (at one place the first pattern's match is the longer one wherever both match: leftmost-first is leftmost-longest)
    rx = re.compile(b"|".join(b"(?:" + p + b")" for p in CUT_PATTERNS))
    per_class = [[m.group() for m in rx.finditer(u)] for u in s.rows.uniq]
    count = np.array([len(m) for m in per_class], dtype=np.int64)[s.rows.inv]
    matches = [m for u in s.rows.inv.tolist() for m in per_class[u]]
    # neighbours in one string that a decoder reading on would decode otherwise
    cut = sum(1 for u, ms in zip(s.rows.uniq, per_class) for a, b in zip(ms, ms[1:])
              if a + b in u and dp.decode(dp.PERCENT, 0, a + b)[0] != dp.decode(dp.PERCENT, 0, a)[0] + dp.decode(dp.PERCENT, 0, b)[0])
    assert cut >= 4 and {b"x%4", b"1y", b"100%4", b"%2", b"5%3"} <= set(matches)
    rows = s.rows.take(np.repeat(np.arange(s.rows.n), count), strs=matches)
    xs = s.sc.extract_set(CUT_PATTERNS)
    ext = s.res.extract_device(xs)
    check_records(s.sc, ext, rows, True, s.name + ": the extraction")
    d = ext.decode_device(kind, utf16le=utf16le)
    check_decode(s, ext, d, kind, utf16le, rows)
    d.decode_words.free(); d.free(); ext.free(); xs.free()


@pytest.mark.parametrize("kind,utf16le", ALL)
def test_a_source_in_which_nothing_decodes_is_copied(sources, kind, utf16le):
    s = sources("plain")
    outs = dp.decoded(dp.KINDS[kind], flags_of(utf16le), s.rows.strs)
    assert not any(w for _, w in outs)                  # (every line of result_plant holds a ':' or an '=' in its middle, and no '%')
    d = s.res.decode_device(kind, utf16le=utf16le)
    check_decode(s, s.res, d, kind, utf16le)
    check_records(s.sc, d, s.rows, True, s.name + ": a copy")
    assert d.decode_info == dict(findings=s.rows.n, decoded=0, text=0, wide=0, bytes_in=int(s.rows.length.sum()), bytes_out=int(s.rows.length.sum()))
    assert not words_of(s.sc, d.decode_words, s.res).any()
    got, want = printed_on_device(s.sc, d), s.rows.text()
    assert got == want
    d.decode_words.free(); d.free()


def test_refusals_are_decided_before_anything_is_launched(merged):
    s, L = merged, sx.lib()
    for kind, flags in ((0, 0), (4, 0), (dp.BASE64, 2), (dp.HEX, 0x80000001)):
        out, words, info = C.c_void_p(0xDEAD0), C.c_void_p(0xDEAD0), sx.DecodeInfo()
        assert L.sx_result_decode_device(s.sc.h, s.res.h, kind, flags, C.byref(out), C.byref(words), C.byref(info)) == sx.SX_E_INVALID
        assert out.value is None and words.value is None and b"SX_DECODE" in L.sx_last_error(s.sc.h)
    with pytest.raises(ValueError):
        s.res.decode_device("base32")
    check_records(s.sc, s.res, s.rows, True, s.name + ": the source, intact")
    # the words and the info are optional
    out = C.c_void_p()
    assert L.sx_result_decode_device(s.sc.h, s.res.h, dp.HEX, 0, C.byref(out), None, None) == sx.SX_OK and out.value
    d = sx.Result(s.sc, out)
    assert len(d) == s.rows.n
    # the blocks take turns: `d` lies in the block that the second selection from now writes
    e1 = s.res.decode_device("hex")
    out, words = C.c_void_p(0xDEAD0), C.c_void_p(0xDEAD0)
    assert L.sx_result_decode_device(s.sc.h, d.h, dp.HEX, 0, C.byref(out), C.byref(words), None) == sx.SX_E_STATE
    assert out.value is None and words.value is None and b"two calls ago" in L.sx_last_error(s.sc.h)
    e1.decode_words.rebind(e1).free()          # (the refused call aged nothing: e1 is still there)
    e1.decode_words.free(); e1.free(); d.free()
    # a result in host memory
    host = sx.Scanner(fp.ms1(), device=0)
    try:
        res = host.scan(dp.buffer(65), file_id=1)
        with pytest.raises(sx.SxError) as e:
            res.decode_device("base64")
        assert e.value.code == sx.SX_E_STATE
        res.free()
    finally:
        host.close()


@pytest.mark.parametrize("kind,utf16le", ALL)
def test_lines_of_1024_characters(sources, kind, utf16le):
    s = sources("long")
    d = s.res.decode_device(kind, utf16le=utf16le)
    _, words = check_decode(s, s.res, d, kind, utf16le)
    longest = int((words >> np.uint64(32)).max())
    assert longest == {("base64", False): 768, ("base64", True): 384, ("hex", False): 512, ("hex", True): 256}.get((kind, utf16le), longest)
    if kind == "percent" and not utf16le:
        assert longest == 1022                 # the line whose escape is its last three bytes
    d.decode_words.free(); d.free()


def test_a_packed_string_that_outgrows_its_record_is_refused_and_nothing_is_written(sources):
    s = sources("limit")
    big = max(s.rows.strs, key=len)
    out, word = dp.decode(dp.PERCENT, dp.UTF16LE, big)
    assert len(big) <= 0xFFFF < len(out) == word >> 32 and all(g[4] for g in s.res.device_segments())
    before = s.res.select_device(b"limit")              # a selection in the block whose turn is NOT next
    n_before = len(before)
    assert n_before >= 2
    with pytest.raises(sx.SxError) as e:
        s.res.decode_device("percent", utf16le=True)
    assert e.value.code == sx.SX_E_INVALID and b"65535" in sx.lib().sx_last_error(s.sc.h)
    # nothing was written and nothing aged: the source prints, and so does the earlier selection after one more selection
    got, want = printed_on_device(s.sc, s.res), s.rows.text()
    assert got == want
    other = s.res.select_device(b"short")
    assert len(before.findings()) == n_before
    other.free(); before.free()
    # without the flag every output fits
    d = s.res.decode_device("percent")
    check_decode(s, s.res, d, "percent", False)
    assert d.decode_info["decoded"] >= 2
    d.decode_words.free(); d.free()
