"""sx_result_measure_device where only the device can go wrong, over the lines tests/measure_plant.py plants for it (tests/test_measure_plant.py
asserts on the CPU what they hold).  tests/test_gpu_measure_device.py never makes a wavefront of measure_wide_kernel measure a second
string, never lists a wide record from the narrow kernel's second trip, and puts few strings at the wide lanes' word edges:

    trip       measure_plant.wide_trip_lines(W), W = CUs x kMeasureWideGroupsPerCu x kRowsWaves read from the sources and the device:
               ONE segment that lists more than 2 W wide records, so every wavefront of the wide kernel takes two strings and some take
               three — the zeroing in measure_wide_finish_lane, the fence and wave_barrier behind it that order a lane's zero-stores
               before the other lanes' next LDS atomics, and chars / ascii_n summed over trips before the one atomicAdd
    late       measure_plant.late_wide_lines(R), R the records of one trip of measure_narrow_kernel: the kernel's second trip has two
               wavefronts that list wide records — lanes 0, 1 and 63 of the one, lane 0 of the other — behind the one entry of trip 1;
               and 64 characters in 255 and in 256 bytes next to each other on the wave path
    edge       measure_plant.word_edge_lines(): wide strings of 33, 63, 64, 65, 127, 128 and 129 aligned words, 64 and 65 at every head
               alignment, and every pair (head alignment, bytes in the last word) among the wide and among the narrow strings — checked
               on the records that lie in HBM, not on the plan alone; and again where a selection and an order laid the strings
    reset      measure_plant.reset_lines(): a segment without a wide string directly behind a segment of nothing else — only the
               cursor's reset keeps the wide kernel from taking the list of the segment before —; and the call between the other users
               of the context's table (sx_ctx::d_distinct), distinct_device and seen_device, which leave it dirty

Every expected word is measure_plant.measure() — the rule in Python — of the oracle's string (result_plant.expected()); no value comes
from a product Scanner."""
import numpy as np
import pytest

import long_plant as lp
import measure_plant as mp
import result_plant as rp
import stringsext_amd as sx
from test_gpu_fold_edges import PARTS, make_from
from test_gpu_measure_device import measured, narrow_trip, wide_of
from test_gpu_result_long_strings import check_sel
from test_gpu_result_on_device_multi import F16, F32
from test_gpu_result_strides import COUNTED, SeenModel, check_records, constant, same, words_of

pytestmark = pytest.mark.gpu

FIRST, REPEATED, SEEN, SHIFT = sx.SX_DISTINCT_FIRST, sx.SX_DISTINCT_REPEATED, sx.SX_DISTINCT_SEEN, sx.SX_DISTINCT_COUNT_SHIFT


def wide_grid():
    """W: the wavefronts of measure_wide_kernel's grid, once a segment has that many records"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count      # hipDeviceAttributeMultiprocessorCount: what rows_grid asks
    assert cus > 0
    return cus * constant("kMeasureWideGroupsPerCu") * constant("kRowsWaves")


MAKERS = {
    "trip": lambda: make_from("wide trip", "merged", lp.msl2(), lp.buffer(mp.wide_trip_lines(wide_grid()))),
    "late": lambda: make_from("late", "wave", lp.msw(), lp.buffer(mp.late_wide_lines(narrow_trip()))),
    "edge": lambda: make_from("word edges", "merged", lp.msl2(), lp.buffer(mp.word_edge_lines())),
    "reset": lambda: make_from("reset", "merged", lp.msl2(), lp.buffer(mp.reset_lines()), PARTS),
}


@pytest.fixture(scope="module")
def sources():
    made = {}

    def get(name):
        if name not in made:
            made[name] = MAKERS[name]()
        return made[name]
    yield get
    for s in made.values():
        s.close()


def placed(sc, res):
    """(head alignment, str_len) of every record, from the records and the arenas' addresses in HBM"""
    head, length = [], []
    for recs_at, n, arena_at, _, packed, _ in res.device_segments():
        recs = np.frombuffer(sc.download(recs_at, n * (16 if packed else 32)), dtype=F16 if packed else F32)
        head.append((arena_at + recs["str_off"].astype(np.int64)) % 8)
        length.append(recs["str_len"].astype(np.int64))
    return np.concatenate(head), np.concatenate(length)


# ---- 1. three strings per wide wavefront

def test_three_strings_per_wide_wavefront(sources):
    w = wide_grid()
    s = sources("trip")
    assert len(s.res.device_segments()) == 1 and s.rows.n >= w                 # one list, and the grid is as large as the device holds
    m, want = measured(s)
    assert m.info["wide"] == 2 * w + 4 > 2 * w and m.info["wide"] < s.rows.n and m.info["ascii"] == s.rows.n
    m.free()


# ---- 2. a list written in the narrow kernel's second trip

def test_wide_records_listed_in_the_narrow_kernels_second_trip(sources):
    r = narrow_trip()
    s = sources("late")
    wide = [0] + [r + p for p in mp.LATE_WIDE]
    assert s.rows.n == r + mp.LATE_TAIL and np.nonzero(s.rows.length.astype(np.int64) > mp.NARROW_MAX)[0].tolist() == wide
    _, length = placed(s.sc, s.res)
    assert np.nonzero(length > mp.NARROW_MAX)[0].tolist() == wide and length[:2].tolist() == [256, 255]
    assert s.rows.strs[:2] == [mp.SMALLEST_WIDE, mp.LARGEST_NARROW]
    m, want = measured(s)
    assert m.info["wide"] == len(wide) == 5 and 0 < m.info["ascii"] < s.rows.n and m.info["chars"] < m.info["bytes"]
    assert [int(x) >> 32 for x in want[:2]] == [64, 64]
    m.free()


# ---- 3. word counts and ends

def test_every_word_count_and_every_pair_of_ends(sources):
    s = sources("edge")
    assert len(s.res.device_segments()) == 1
    head, length = placed(s.sc, s.res)
    planned = s.rows.length.astype(np.int64)
    same(length, planned, s.name + ": str_len")
    same(head, (np.cumsum(planned) - planned) % 8, s.name + ": the strings' places modulo 8")
    mp.word_edges_complete(head.tolist(), length.tolist())
    m, want = measured(s)
    assert 0 < m.info["wide"] < s.rows.n
    m.free()


def test_the_words_of_a_selection_and_of_an_order_of_the_word_edges(sources):
    s = sources("edge")
    head, length = placed(s.sc, s.res)
    mask = s.rows.mask(lambda x: b"mmap" in x)
    assert 0 < mask.sum() < s.rows.n
    sel = s.res.select_device(b"mmap")
    kept = check_sel(s, s.res, sel, mask)
    kept_len = kept.length.astype(np.int64)
    assert (kept_len > mp.NARROW_MAX).sum() > 100 and (kept_len <= mp.NARROW_MAX).sum() > 100
    new_head, new_len = placed(s.sc, sel)
    same(new_len, kept_len, s.name + ": the selection's str_len")
    assert (new_head != head[mask]).sum() > kept.n // 2                                              # the strings lie at new places
    assert {int(h) for h, n in zip(new_head, new_len) if n > mp.NARROW_MAX} == set(range(8))
    m, _ = measured(s, sel, kept)
    m.free(); sel.free()
    order = sorted(range(s.rows.n), key=lambda i: s.rows.strs[i])                                     # (sorted() is stable: ties keep print order)
    rows = s.rows.take(np.array(order, dtype=np.int64))
    out = s.res.order_device("string")
    check_records(s.sc, out, rows, True, s.name + ": in order")
    new_head, new_len = placed(s.sc, out)
    assert (new_head != head[order]).sum() > s.rows.n // 2
    counts, _, _, _ = mp.word_edges(new_head.tolist(), new_len.tolist())
    assert {v for v, _ in counts} >= set(mp.WORD_COUNTS) and len(out.device_segments()) == 1
    m, _ = measured(s, out, rows)
    m.free(); out.free()


# ---- 4. a segment without wide strings behind one of nothing else

def test_a_segment_without_wide_strings_behind_one_of_nothing_else(sources):
    s = sources("reset")
    per_seg = wide_of(s)
    pattern = "".join("w" if w.all() else "m" if w.any() else "n" for w in per_seg)
    assert pattern == "wwwwwwwwnn", (pattern, [len(w) for w in per_seg])
    assert [len(w) for w in per_seg] == mp.merge_parts(s.rows.position.tolist(), int(s.rows.length.sum()), len(lp.buffer(mp.reset_lines())))
    m, want = measured(s)
    assert m.info["wide"] == sum(int(w.sum()) for w in per_seg) > 2 * 1024 and s.rows.n - m.info["wide"] > 2 * 1024
    m.free()


# ---- 5. behind and in front of the table's other users

def test_between_the_calls_that_share_the_contexts_table(sources):
    """distinct_device and seen_device keep their hash tables where measure_device keeps its totals, cursor and list: each call has to
    make the table its own, whatever the call before left there"""
    s = sources("reset")
    distinct = rp.distinct_model(s.rows.strs, FIRST, REPEATED, SHIFT)

    def distinct_call():
        lab = s.res.distinct_device()
        same(words_of(s.sc, lab, s.res), distinct[0], s.name + ": distinct words", s.rows.strs)
        assert {k: lab.info[k] for k in ("findings", "distinct", "repeated")} == distinct[1], (lab.info, distinct[1])
        lab.free()

    distinct_call()
    measured(s)[0].free()
    distinct_call()
    full = SeenModel()
    full.expect(distinct)
    cap = full.held_info()
    ss, model = s.sc.seen_set(cap["strings"], cap["bytes"]), SeenModel()
    try:
        for round_ in range(2):
            want, want_info = model.expect(distinct)
            lab = s.res.seen_device(ss)
            same(words_of(s.sc, lab, s.res), want, "%s: seen words, call %d" % (s.name, round_), s.rows.strs)
            assert {k: lab.info[k] for k in COUNTED} == want_info, (lab.info, want_info)
            assert bool((want & np.uint64(SEEN)).all()) == (round_ == 1)
            lab.free()
            measured(s)[0].free()
        info = ss.info()
        assert dict(strings=info["strings"], bytes=info["bytes"]) == model.held_info()
    finally:
        ss.free()
    distinct_call()
