"""sx_result_measure_device (Result.measure_device): what the strings of a result that lies in HBM look like — entropy, distinct bytes,
class bits, characters —, measured on the device, and what the selections and the order make of the words.

The kernels' split: a LANE measures a string of at most 255 bytes (measure_narrow_kernel, one-byte counters in LDS), a WAVEFRONT a
longer one (measure_wide_kernel, from the list the narrow kernel leaves).  The edges, and the source that stands on each:
    record counts   `wave k` / `lane k`: fold_plant's lines, one UTF-8 Mission — packed records on the wave path, unpacked ones on the
                    lane-per-region replay —, k = 1, 63, 64, 65, 129; `trip`: R + 1 records in one segment, R = CUs x
                    kMeasureGroupsPerCu x kMeasureWaves x 64 read from the sources as tests/test_gpu_result_strides.py reads its
                    constants — record R is the one record of the narrow kernel's second trip, on the lane that had record 0, and its
                    bytes are that record's plus one; `merged`: `-e ascii -e utf-8` under SX_MERGE_PART_FINDINGS=1024, several packed
                    segments
    255 | 256       `edges` (long_plant.msl2(), -q 1024, parts of 1024 findings) and `one` (long_plant.msl1(), -q 255, unpacked):
                    lines of 254, 255, 256 and 257 bytes; 600 x `7` — a count above 255, entropy 0 —; a wide line of every printable
                    value; wide records at the first and the last place of a wavefront; more than 64 wide records in a row (the list's
                    reserve); a segment without a wide string and one of nothing else; a narrow string of `q` directly behind a wide
                    one of nothing else — the two kernels count in counters of their own, so this shows no counter left behind: it
                    pins the narrow lane's word beside a wide neighbour; a lane's own clearing is `trip`'s, and the wide wavefront's,
                    which needs a wavefront that measures a second string, is tests/test_gpu_measure_edges.py's —; `limit`
                    (long_plant.limit_ms()): 16 000 and 64 000 bytes
    UTF-8           fold_plant's lines in every source of the first kind; `cuts`: an extraction that cuts characters in two, as
                    tests/test_gpu_fold_edges.py makes it — chars counts the lead byte only

Every expected word is measure_plant.measure() — the rule in Python — of the oracle's string (result_plant.expected()); no value comes
from a product Scanner.  SX_MEASURE_CONTROL: no Mission lets a control byte into a string, so that bit stays pinned on the host only
(tests/test_measure_core.py)."""
import ctypes as C

import numpy as np
import pytest

import fold_plant as fp
import long_plant as lp
import measure_plant as mp
import result_plant as rp
import stringsext_amd as sx
from test_gpu_fold_device import SMALL, make
from test_gpu_fold_edges import PARTS, extracted, make_from
from test_gpu_result_long_strings import check_sel
from test_gpu_result_strides import check_records, constant, picked, printed_on_device, same, words_of

pytestmark = pytest.mark.gpu

MERGED_LINES = 3000


def narrow_trip():
    """R: the records of one segment that fill one trip of measure_narrow_kernel"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count      # hipDeviceAttributeMultiprocessorCount: what rows_grid asks
    assert cus > 0 and constant("kSelectRecs") == 64 and constant("kMeasureNarrowMax") == mp.NARROW_MAX
    return cus * constant("kMeasureGroupsPerCu") * constant("kMeasureWaves") * 64


MAKERS = {
    "merged": lambda: make("merged", MERGED_LINES),
    "trip": lambda: make_from("trip", "wave", fp.ms1(), lp.buffer(mp.second_trip_lines(narrow_trip()))),
    "edges": lambda: make_from("edges", "merged", lp.msl2(), lp.buffer(mp.edge_lines()), PARTS),
    "one": lambda: make_from("one", "lane", lp.msl1(), lp.buffer(mp.one_edge_lines())),
    "limit": lambda: make_from("limit", "merged", lp.limit_ms(), lp.buffer(lp.limit_lines())),
    "cuts": lambda: make_from("cuts", "lane", fp.ms1(), lp.buffer(fp.split_lines())),
}


@pytest.fixture(scope="module")
def sources():
    made = {}

    def get(name, k=None):
        if (name, k) not in made:
            made[name, k] = make(name, k) if k else MAKERS[name]()
        return made[name, k]
    yield get
    for s in made.values():
        s.close()


def lying(sc, res):
    """every segment's records and strings, as bytes"""
    return [(sc.download(g[0], g[1] * (16 if g[4] else 32)), sc.download(g[2], g[3])) for g in res.device_segments()]


def want_words(strs):
    return np.array([mp.measure(x) for x in strs], dtype=np.uint64)


def measured(s, res=None, rows=None):
    """res.measure_device(), checked: every word, the info, the host twin on every string, the source byte for byte what it was, and
    a selection made before still printing what it printed — three calls age nothing.  Returns (the Labels, the words)"""
    res, rows = res or s.res, rows or s.rows
    before = lying(s.sc, res)
    first = rows.strs[0][:4]
    sel = res.select_device(first)
    text = printed_on_device(s.sc, sel)
    if rows.raw is not None:
        assert text == rows.take(rows.mask(lambda x: first in x)).text(), s.name
    for _ in range(2):
        res.measure_device().free()
    m = res.measure_device()
    want = want_words(rows.strs)
    same(words_of(s.sc, m, res), want, s.name + ": the words", rows.strs)
    assert m.info == mp.info(rows.strs), (s.name, m.info, mp.info(rows.strs))
    for x in set(rows.strs):
        assert sx.measure(x) == mp.measure(x), (s.name, x[:60])
    assert lying(s.sc, res) == before, s.name
    assert printed_on_device(s.sc, sel) == text, s.name
    sel.free()
    return m, want


@pytest.mark.parametrize("k", SMALL)
@pytest.mark.parametrize("kind", ["wave", "lane"])
def test_the_words_of_one_mission_around_a_wavefront(sources, kind, k):
    s = sources(kind, k)
    m, want = measured(s)
    assert m.info["findings"] == k and m.info["wide"] == 0 and (k < 63 or 0 < m.info["ascii"] < k and m.info["chars"] < m.info["bytes"])
    m.free()


def test_the_words_of_merged_missions_in_several_segments(sources):
    s = sources("merged")
    assert len(s.res.device_segments()) >= 3
    m, want = measured(s)
    assert 0 < m.info["ascii"] < s.rows.n and m.info["chars"] < m.info["bytes"]
    m.free()


def test_one_record_in_the_second_trip_with_the_first_trips_bytes_plus_one(sources):
    r = narrow_trip()
    s = sources("trip")
    assert s.rows.n == r + 1 and sorted(s.rows.strs[r]) == sorted(s.rows.strs[0] + b"!")
    m, want = measured(s)
    # what a lane that kept record 0's counts would say of record r: twice the bytes
    assert want[r] != mp.measure(s.rows.strs[0] + s.rows.strs[r]) and want[r] != want[0]
    m.free()


def wide_of(s):
    """per segment of s.res the bool array `this record's string is wide`"""
    at, out = 0, []
    wide = s.rows.length.astype(np.int64) > mp.NARROW_MAX
    for g in s.res.device_segments():
        out.append(wide[at:at + g[1]])
        at += g[1]
    return out


def test_both_sides_of_255_bytes_in_packed_parts(sources):
    s = sources("edges")
    per_seg = wide_of(s)
    assert len(per_seg) >= 5
    assert any(not w.any() for w in per_seg) and any(w.all() for w in per_seg)                        # a segment without, one of nothing else
    places = {int(i) % 64 for w in per_seg for i in np.nonzero(w)[0]}
    assert {0, 63} <= places                                                                          # a wavefront's first and last record
    joined = ["".join("w" if x else "n" for x in w) for w in per_seg]
    assert any("w" * 70 in j and "n" in j for j in joined)                                            # more than a wavefront's worth in a row
    for line in (mp.SEVENS, mp.PRINTABLE, b"7" * 255, b"7" * 256) + tuple(mp.ascii_edge(n) for n in mp.EDGE_LENGTHS):
        assert line in s.rows.strs
    at = s.rows.strs.index(b"q" * 400)
    assert s.rows.strs[at + 1] == mp.LEFTOVER and mp.measure(mp.LEFTOVER) != mp.measure(mp.LEFTOVER + b"q" * 400)
    m, want = measured(s)
    assert m.info["wide"] == sum(int(w.sum()) for w in per_seg) > 2048 and m.info["ascii"] == s.rows.n
    assert want[s.rows.strs.index(mp.SEVENS)] == mp.DIGIT | 1 << 16 | 600 << 32
    m.free()


def test_both_sides_of_255_bytes_in_unpacked_records(sources):
    s = sources("one")
    assert s.rows.strs == mp.one_edge_lines() and not any(g[4] for g in s.res.device_segments())
    m, want = measured(s)
    assert 20 <= m.info["wide"] < s.rows.n and 0 < m.info["ascii"] < s.rows.n and m.info["chars"] < m.info["bytes"]
    assert [int(w) >> 32 for w in want[:4]] == [254, 255, 255, 254]
    m.free()


def test_strings_of_16000_and_64000_bytes(sources):
    s = sources("limit")
    assert {16000, 64000} <= set(s.rows.length.tolist())
    m, want = measured(s)
    assert m.info["wide"] == int((s.rows.length > 255).sum()) >= 6
    assert {int(w) >> 32 for w, n in zip(want, s.rows.length) if n == 64000} == {16000}               # four bytes a character
    m.free()


def test_characters_cut_in_two_by_an_extraction(sources):
    s = sources("cuts")
    ext, rows = extracted(s)
    ends_in_lead = [x for x in rows.strs if x[-1] >= 0xC2]
    begins_in_tail = [x for x in rows.strs if 0x80 <= x[0] <= 0xBF]
    assert len(ends_in_lead) > 10 and len(begins_in_tail) > 10
    assert all(mp.measure(x) >> 32 == sum(1 for b in x if not 0x80 <= b <= 0xBF) for x in ends_in_lead + begins_in_tail)
    assert mp.measure(b"EN8\xd0") >> 32 == 4 and mp.measure(b"\xba") >> 32 == 0                       # the lead byte counts, a lone tail does not
    m, want = measured(s, ext, rows)
    assert m.info["chars"] == sum(int(w) >> 32 for w in want)
    m.free(); ext.free()


# ---- what the selections and the order make of the words

@pytest.mark.parametrize("name", ["merged", "edges"])
def test_select_by_a_range_of_entropy_and_of_characters(sources, name):
    s = sources(name)
    want = want_words(s.rows.strs)
    m = s.res.measure_device()
    ent, chars = (want & np.uint64(0xFFFF)).astype(np.int64), (want >> np.uint64(32)).astype(np.int64)
    lo = int(np.median(ent)) + 1
    for shift, bits, a, b, mask in ((sx.SX_MEASURE_ENTROPY_SHIFT, 16, lo, 65535, ent >= lo), (sx.SX_MEASURE_CHARS_SHIFT, 32, 32, (1 << 32) - 1, chars >= 32),
                                    (sx.SX_MEASURE_CHARS_SHIFT, 32, 255, 256, (chars >= 255) & (chars <= 256)),
                                    (sx.SX_MEASURE_DISTINCT_SHIFT, 9, 0, 9, ((want >> np.uint64(16)) & np.uint64(0x1FF)).astype(np.int64) <= 9)):
        assert name == "merged" and bits == 32 and a == 255 or 0 < mask.sum() < s.rows.n, (shift, a, b)
        sel = s.res.select_range_device(m, shift, bits, a, b)
        check_sel(s, s.res, sel, mask)
        sel.free()
    m.free()


def test_select_by_the_class_bits(sources):
    s = sources("merged")
    want = want_words(s.rows.strs)
    m = s.res.measure_device()
    for masks in (dict(none=sx.SX_MEASURE_HIGH | sx.SX_MEASURE_SPACE), dict(any=sx.SX_MEASURE_UPPER | sx.SX_MEASURE_DIGIT),
                  dict(all=sx.SX_MEASURE_LOWER | sx.SX_MEASURE_DIGIT, none=sx.SX_MEASURE_HIGH), dict(any=sx.SX_MEASURE_CONTROL)):
        mask = picked(want, masks.get("any", 0), masks.get("all", 0), masks.get("none", 0))
        assert (0 < mask.sum() < s.rows.n) == (masks != dict(any=sx.SX_MEASURE_CONTROL)), masks
        sel = s.res.select_device(m, **masks)
        check_sel(s, s.res, sel, mask)
        sel.free()
    m.free()


def test_the_hundred_most_random_strings_in_print_order_among_equals(sources):
    s = sources("merged")
    want = want_words(s.rows.strs)
    ent = (want & np.uint64(0xFFFF)).astype(np.int64)
    order = sorted(range(s.rows.n), key=lambda i: -int(ent[i]))[:100]                                 # (sorted() is stable: ties keep print order)
    assert len({int(ent[i]) for i in order}) < 100                                                    # there are ties among them
    m = s.res.measure_device()
    out = s.res.order_device("field", m, shift=0, bits=16, descending=True, limit=100)
    check_records(s.sc, out, s.rows.take(np.array(order, dtype=np.int64)), True, s.name + ": by entropy")
    assert out.order_info["findings"] == s.rows.n and out.order_info["kept"] == 100
    out.free(); m.free()


def test_the_words_of_a_fold_rebound_to_its_source(sources):
    s = sources("merged")
    fold = s.res.fold_device()
    m, want = measured(s, fold, s.frows)
    plain = want_words(s.rows.strs)
    upper = np.uint64(sx.SX_MEASURE_UPPER)
    assert ((want & upper) == 0).all() and ((plain & upper) != 0).sum() > 100                         # the fold leaves no 'A'..'Z'
    distinct, plain_distinct = ((want >> np.uint64(16)) & np.uint64(0x1FF)).astype(np.int64), ((plain >> np.uint64(16)) & np.uint64(0x1FF)).astype(np.int64)
    mask = distinct <= 12
    assert 0 < mask.sum() < s.rows.n and (mask != (plain_distinct <= 12)).sum() > 10                  # the fold's words, not the source's
    bound = m.rebind(s.res)
    sel = s.res.select_range_device(bound, sx.SX_MEASURE_DISTINCT_SHIFT, 9, 0, 12)
    check_sel(s, s.res, sel, mask)                                                                    # the ORIGINAL strings
    sel.free(); bound.free(); m.free(); fold.free()


def test_refusals(sources):
    s, other, L = sources("merged"), sources("wave", 65), sx.lib()
    out, info = C.c_void_p(0xDEAD0), sx.MeasureInfo()
    for flags in (1, 0x80000000):
        assert L.sx_result_measure_device(s.sc.h, s.res.h, flags, C.byref(out), C.byref(info)) == sx.SX_E_INVALID and out.value is None
    assert L.sx_result_measure_device(s.sc.h, s.res.h, 0, None, None) == sx.SX_E_INVALID
    # labels of another result
    m, mo = s.res.measure_device(), other.res.measure_device()
    for call in (lambda: s.res.select_device(mo, any=1), lambda: s.res.select_range_device(mo, 0, 16, 0, 65535),
                 lambda: other.res.order_device("field", m, shift=0, bits=16)):
        with pytest.raises(sx.SxError) as e:
            call()
        assert e.value.code == sx.SX_E_INVALID
    sel = s.res.select_device(b"a")
    with pytest.raises(sx.SxError) as e:
        sel.select_device(m, any=sx.SX_MEASURE_LOWER)                # the same context, another result
    assert e.value.code == sx.SX_E_INVALID
    sel.free(); m.free(); mo.free()
    # a result in host memory
    host = sx.Scanner(fp.ms1(), device=0)
    try:
        res = host.scan(fp.buffer(65), file_id=1)
        assert len(res) == 65
        out = C.c_void_p(0xDEAD0)
        assert L.sx_result_measure_device(host.h, res.h, 0, C.byref(out), None) == sx.SX_E_STATE and out.value is None
        assert b"host memory" in L.sx_last_error(host.h)
        with pytest.raises(sx.SxError) as e:
            res.measure_device()
        assert e.value.code == sx.SX_E_STATE
        res.free()
    finally:
        host.close()
