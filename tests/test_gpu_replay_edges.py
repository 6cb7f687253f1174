"""Stage B, one lane per region (stringsext_amd/csrc/sx_replay_dev.hip), on the planted inputs of tests/replay_plant.py: every case
sits in windows of its own, so a failure names the case that was planted there, not a byte offset of a diff.  Every scan is compared
finding by finding with the oracle's findings (position, precision, completes_previous, Mission, slice index, string) and then as
printed text with the oracle's command line; no expected value comes from a product Scanner.  tests/test_replay_plant.py proves on
the CPU that the plants are what they claim."""
import re

import pytest

import refconfig as rc
import replay_plant as rp
import stringsext_amd as sx
import sxo_binding as sxo
from test_sharded_gloo import oracle_findings

pytestmark = pytest.mark.gpu

_oracle = {}


def oracle(plant):
    """(findings, text) of the oracle, once per plant"""
    key = id(plant.data)
    if key not in _oracle:
        ms = rc.missions(**plant.flags)
        _oracle[key] = (plant.data, oracle_findings(ms, plant.data), sxo.run_cli(ms, [plant.data], radix="x"))
    return _oracle[key][1:]


def scan(plant, monkeypatch, env=None, chunk=None):
    """-> (findings, text, fast_regions, general_regions) of a device replay without the wave kernels; the records are joined on the
    device whatever their number (a list joined on the host is neither cut into pieces nor replayed in slabs)"""
    env = dict(env or {}, SX_WAVE_REPLAY="0", SX_DEVICE_JOIN_MIN="1")
    for k in ("SX_FAST_REPLAY", "SX_NO_PIECES", "SX_SLABS", "SX_STITCH_BLOCK", "SX_REPLAY_CACHE_MIB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = sx.Scanner(rc.missions(**plant.flags), device=0, device_replay=True)
    found, out = [], bytearray(sx.OUTPUT_BOM)
    step = chunk or max(len(plant.data), 1)
    try:
        for off in range(0, len(plant.data), step):
            res = sc.scan(plant.data[off:off + step], file_id=1)
            found += [(f["position"], f["precision"], f["s"], f["completes"], f["mission_id"], f["slice_index"] + off // rp.SLICE)
                      for f in res.findings()]     # (a result counts its slices from its chunk's first one)
            out += res.printed(n_inputs=1, radix="x")
            res.free()
        st = sc.stats()
        assert st.wave_windows == 0
        return found, bytes(out) + b"\n", st.fast_regions, st.general_regions
    finally:
        sc.close()


def first_line_that_differs(plant, got, want):
    """-> (line number, got, want, the case planted where the line's hexadecimal position points)"""
    for k, (g, w) in enumerate(zip(got.split(b"\n") + [None], want.split(b"\n") + [None])):
        if g != w:
            m = re.match(rb"\xef\xbb\xbf|[<> ]*([0-9a-f]+)", w or g or b"")
            return k, g, w, rp.describe(plant, int(m.group(1), 16)) if m and m.group(1) else None


def check(plant, monkeypatch, env=None, chunk=None):
    """the hard criterion: the oracle's findings and text; -> (fast, general)"""
    want, text = oracle(plant)
    got, printed, fast, general = scan(plant, monkeypatch, env, chunk)
    assert got == want, (env, chunk, rp.first_difference(plant, got, want))
    assert printed == text, (env, chunk, first_line_that_differs(plant, printed, text))
    return fast, general


@pytest.mark.parametrize("q,W", rp.PREPASS_GEOMETRY)
def test_prepass_rules_at_every_edge_of_the_window(q, W, monkeypatch):
    plant = rp.prepass_window(q, W)
    fast, general = check(plant, monkeypatch)
    assert (fast, fast + general) == (plant.fast, plant.heads), (fast, general, plant.fast, plant.heads)
    assert check(plant, monkeypatch, {"SX_FAST_REPLAY": "0"}) == (0, 0)
    check(plant, monkeypatch, chunk=8 * rp.SLICE)


@pytest.mark.parametrize("q,W", rp.PIECES_GEOMETRY)
def test_pieces_of_runs_across_window_starts(q, W, monkeypatch):
    plant = rp.pieces(q, W)
    fast, general = check(plant, monkeypatch)
    assert (fast, fast + general) == (plant.fast, plant.heads), (fast, general, plant.fast, plant.heads)
    assert check(plant, monkeypatch, {"SX_FAST_REPLAY": "0"}) == (0, 0)
    whole = rp.pieces(q, W, cut=False)
    assert whole.data == plant.data
    fast, general = check(plant, monkeypatch, {"SX_NO_PIECES": "1"})
    assert (fast, fast + general) == (whole.fast, whole.heads), (fast, general, whole.fast, whole.heads)


def counted(plant, monkeypatch, env=None):
    fast, general = check(plant, monkeypatch, env)
    assert (fast, fast + general) == (plant.fast, plant.heads), (env, fast, general, plant.fast, plant.heads)


@pytest.mark.parametrize("band", [0, 1, 2])
def test_copy_of_the_cached_outputs_in_every_band(band, monkeypatch):
    """replay_copy_cached_kernel<4, 2>, <32, 4> and <64, 4>: heads, bodies and tails at every phase, 1 .. G/2 + 1 findings per region"""
    counted(rp.copy_band(band), monkeypatch)


def test_outputs_of_exactly_a_cache_slot_and_one_more(monkeypatch):
    plant = rp.cache_edge()
    fast, general = check(plant, monkeypatch, {"SX_REPLAY_CACHE_MIB": "0"})
    assert (fast, fast + general) == (plant.extra["fast"], plant.heads), (fast, general, plant.extra["fast"], plant.heads)
    counted(plant, monkeypatch)     # (slots for all)


@pytest.mark.parametrize("block", rp.STITCH_BLOCKS)
def test_void_regions_at_the_edges_of_the_stitch(block, monkeypatch):
    plant = rp.stitch(block)
    env = {"SX_STITCH_BLOCK": str(block)} if block else {}
    counted(plant, monkeypatch, env)
    if block == 7:   # the region the host replays at a chunk's start ends behind the first head of the chunk's list (E0)
        check(plant, monkeypatch, env, chunk=rp.STITCH_CHUNK)


@pytest.mark.parametrize("one_more", [False, True])
def test_a_lane_of_the_bounded_count_grid_takes_a_second_trip(one_more, monkeypatch):
    plant = rp.count_trips(one_more)
    fast, general = check(plant, monkeypatch)
    assert (fast, general) == (0, plant.heads)


@pytest.mark.parametrize("slabs", rp.SLABS)
def test_slab_cuts_next_to_pieces_and_chains(slabs, monkeypatch):
    """SX_SLABS with fewer entries than slabs_wanted asks for replays one slab: rp.slab_plants gives the plants that have enough"""
    for plant in rp.slab_plants(slabs):
        check(plant, monkeypatch, {"SX_SLABS": str(slabs)})
