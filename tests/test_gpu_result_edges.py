"""The operations of tests/test_gpu_result_strides.py on results whose record count lies ON a wavefront edge (64) or a workgroup edge —
256 for the four-wavefront kernels select_match_kernel, select_place_kernel and label_pick_kernel, 512 for the rows kernels — and one
record on either side.  At n % 64 == 0 the selections' extra wavefront lies wholly behind the data, at n % 512 == 0 it opens a
workgroup of its own; select_load_lane gives the lanes behind n an empty string at the end of the last record's, and the scans run over
waves + 1 words.  The sources: tests/result_plant.py prefix(k) scanned with one Mission (k findings), with two Missions (2 k findings,
merged), and the k records that a token planted on exactly k lines of a larger buffer selects — an earlier selection's output as the
source, at the exact count.  Every expected value comes from the oracle's text.  One Scanner per Mission set serves every k.

One Mission's result stays in HBM only where the device wrote it in one block (include/stringsext_amd.h, SX_OPT_RESULT_ON_DEVICE): the
default path replays a buffer of a few hundred runs on the host, and its result is in host memory.  So the one-Mission sources take
the two paths that do write on the device, at EVERY k: "one" the wave path (SX_WAVE_REPLAY=1 as in tests/test_gpu_result_strides.py:
packed records, strings where the writer put them; it takes whole buffers of two windows or more, so prefix(k) is followed by bytes
in which the Mission reads nothing), "replay" the lane-per-region replay (SX_OPT_DEVICE_REPLAY, and SX_WAVE_REPLAY=0 since by density
the buffers of two windows would take the wave path: unpacked records).  The replay's first region is the host's entry part, and a
buffer whose findings all lie in it — prefix(1), prefix(2) — has nothing the device wrote: those two are no "replay" sources."""
import numpy as np
import pytest

import result_plant as rp
import stringsext_amd as sx
from test_gpu_result_strides import (SUBSTRING_CASES, Source, check_records, op_distinct, op_extract, op_label, op_pattern_set, op_printed, op_records,
                                     op_regex_set, op_seen, op_select_all_and_none, op_select_substring, op_tally)

pytestmark = pytest.mark.gpu

EDGES = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513]
LARGER = 2000      # lines of the buffer a token selects k records from
TOKEN = b"{pick}"
QUIET, TWO_WINDOWS = b"\x80", 2 * 4096      # a byte in which `-e ascii` reads no character; the wave path takes buffers of two windows or more
SPECS = [("one", k) for k in EDGES] + [("replay", k) for k in EDGES if k > 2] + [("two", k) for k in (32, 128, 256)] + [("picked", k) for k in EDGES]


@pytest.fixture(scope="module")
def scanners():
    ms1, ms2 = rp.ms1(), rp.ms2()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SX_WAVE_REPLAY", "1")                    # (a context keeps the switches it was created under)
        wave = sx.Scanner(ms1, device=0, result_on_device=True)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SX_WAVE_REPLAY", "0")
        replay = sx.Scanner(ms1, device=0, device_replay=True, result_on_device=True)
    out = {"one": (ms1, wave),
           "replay": (ms1, replay),
           "two": (ms2, sx.Scanner(ms2, device=0, result_on_device=True))}
    out["picked"] = out["one"]
    yield out
    for kind in ("one", "replay", "two"):
        out[kind][1].close()


@pytest.fixture(scope="module", params=SPECS, ids=["%s-%d" % spec for spec in SPECS])
def source(request, scanners):
    """the result of a spec on the device, the oracle's rows for it; a scan with at least one finding stays on the device"""
    kind, k = request.param
    ms, sc = scanners[kind]
    data = rp.with_token(LARGER, k, TOKEN) if kind == "picked" else rp.prefix(k)
    if kind == "one":
        data += QUIET * max(0, TWO_WINDOWS - len(data))
    rows = rp.expected(ms, data)
    sc.reset()                                              # (every buffer is a stream of its own)
    res = sc.scan(data, file_id=1)
    segs = res.device_segments()
    assert len(res) == rows.n == (LARGER if kind == "picked" else k * len(ms)), (kind, k, len(res), rows.n)
    assert len(segs) == 1 and segs[0][0] and segs[0][2] and segs[0][1] == rows.n, [(g[0], g[1], g[2]) for g in segs]
    assert segs[0][4] == (kind != "replay")                 # (the lane-per-region replay's records are sx_finding)
    name = "%s-%d" % (kind, k)
    if kind != "picked":
        s = Source(name, sc, res, rows, ms, back_to_back=kind == "two")
        assert s.sentinel_last
        yield s
        s.close()
        return
    mask = rows.mask(lambda x: TOKEN in x)
    assert mask.sum() == k and mask[0]
    s = Source(name, sc, res.select_device(TOKEN), rows.take(mask), ms, back_to_back=True, remake=lambda: res.select_device(TOKEN))
    assert len(s.res) == k
    yield s
    s.close(); res.free()


def test_records_and_strings_as_they_lie(source):
    op_records(source)


def test_printed_device_is_the_oracles_text(source):
    op_printed(source)


@pytest.mark.parametrize("case", SUBSTRING_CASES)
def test_select_by_substring(source, case):
    op_select_substring(source, case)


def test_select_everything_and_nothing(source):
    op_select_all_and_none(source)


def test_select_by_2000_keywords(source):
    op_pattern_set(source)


def test_select_by_regex(source):
    op_regex_set(source)


def test_extract(source):
    op_extract(source)


def test_tally(source):
    op_tally(source)


def test_labels(source):
    op_label(source)


@pytest.mark.parametrize("nocase", [False, True], ids=["plain", "ignore_case"])
def test_distinct(source, nocase):
    op_distinct(source, nocase)


def test_seen(source):
    op_seen(source)


def test_a_selection_of_exactly_k_is_the_source_of_a_selection_of_exactly_k(source):
    """select everything from the source, and from that again: the count stays on its edge through two selections"""
    res = source.fresh()
    everything = res.select_device(b"\x02\x02", invert=True)
    assert len(everything) == source.rows.n
    again = everything.select_device(b"\x02\x02", invert=True)
    check_records(source.sc, again, source.rows, True, source.name + ": twice selected")
    again.free(); everything.free()
