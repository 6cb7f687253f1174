"""The plants of tests/replay_plant.py are what they claim (no GPU): the oracle gives every case the findings the plant predicts from
the numbers it planted; the device replay core, compiled for the host, says which regions of the stitch plants end where, and the
sequential rule (a region stands iff it begins at or behind the end of the last standing one) makes void exactly the entries the
plants list; the copy plants' means lie in their bands; the trip plants have as many heads as one trip of the grid visits."""
import ctypes as C

import pytest

import refconfig as rc
import replay_plant as rp
import sxo_binding as sxo
from test_sharded_gloo import oracle_findings


def agree(plant):
    got = [(p, pr, s, c) for p, pr, s, c, _, _ in oracle_findings(rc.missions(**plant.flags), plant.data)]
    assert got == plant.expect, rp.first_difference(plant, got, plant.expect)
    return got


def test_the_constants_are_where_the_plants_read_them():
    assert rp.count_grid_cap() == (4096, 64)
    assert [(b[0], b[1]) for b in rp.copy_bands()] == [(96, 4), (640, 32), (None, 64)]
    assert rp.cache_geom_constants() == (160, 4096, 96)
    assert rp.stitch_block_default() == 128
    assert rp.avg_out_bytes_rule() == 32


@pytest.mark.parametrize("q,W", rp.PREPASS_GEOMETRY)
def test_oracle_gives_every_prepass_case_the_predicted_finding(q, W):
    plant = rp.prepass_window(q, W)
    agree(plant)
    assert 0 < plant.fast < plant.heads <= len(plant.runs)
    # 0xFF at every offset of a window, a six-byte run behind each: one finding each, those across the window start at it
    first = [f for f in plant.expect if f[0] < plant.notes[W][0]]
    assert len(first) == W and [f[1] for f in first].count("Before") > 0


@pytest.mark.parametrize("q,W", rp.PIECES_GEOMETRY)
def test_oracle_gives_every_piece_case_the_predicted_findings(q, W):
    plant = rp.pieces(q, W)
    agree(plant)
    whole = rp.pieces(q, W, cut=False)
    assert whole.data == plant.data and whole.expect == plant.expect
    assert plant.heads > whole.heads and plant.fast > whole.fast == 0 and any(r[3] for r in plant.runs) and not any(r[3] for r in whole.runs)


@pytest.mark.parametrize("band", [0, 1, 2])
def test_copy_band_means_lie_a_factor_of_two_inside_their_band(band):
    plant = rp.copy_band(band)
    got = agree(plant)
    lower, upper = plant.extra["band"]
    mean = (len(got) * rp.avg_out_bytes_rule() + sum(len(f[2].encode("utf-8")) for f in got)) // plant.heads
    assert mean == plant.extra["mean"] and 2 * lower <= mean and (upper is None or 2 * mean <= upper), (mean, lower, upper)
    assert not any(r[3] for r in plant.runs)                       # no pieces: a region is a chain of strings
    G = plant.extra["G"]
    _, cap_f, cap_b = rp.cache_geom(rp.cache_arena_bytes(len(plant.runs)), plant.heads)
    assert set(plant.extra["findings"].values()) == {1, 2, 3, G // 2, G // 2 + 1} and cap_f > G // 2 + 1
    for pos, n in plant.extra["findings"].items():
        end = min(p for p, _ in plant.notes + [(len(plant.data), "")] if p > pos)
        mine = [f for f in got if pos <= f[0] < end]
        assert len(mine) == n and sum(len(f[2].encode("utf-8")) for f in mine) <= cap_b, (pos, n)
    assert max(len(f[2].encode("utf-8")) for f in got) > 4 * G
    # the copy of a region's strings: its destination is where the strings of the regions before it end (they all stand); the head
    # are the bytes up to the next dword, the tail what is left behind whole dwords
    bounds = sorted(p for p, _ in plant.notes) + [len(plant.data)]
    pairs, short, at, k = set(), 0, 0, 0
    for lo, hi in zip(bounds, bounds[1:]):
        nb = 0
        while k < len(got) and got[k][0] < hi:
            nb += len(got[k][2].encode("utf-8"))
            k += 1
        head = min(-at % 4, nb)
        pairs.add((at % 4, (nb - head) % 4))
        short += nb < -at % 4
        at += nb
    assert k == len(got) and len(pairs) == 16, sorted(pairs)
    if band == 0:
        assert min(len(f[2].encode("utf-8")) for f in got) == 2 and short > 0    # head > nb


def test_cache_edge_regions_are_exactly_a_slot_and_one_more():
    plant = rp.cache_edge()
    got = agree(plant)
    slot, cap_f, cap_b = plant.extra["slot"]
    assert (slot, cap_f, cap_b) == rp.cache_geom(rp.cache_arena_bytes(len(plant.runs), 0), plant.heads) == (160, 2, 96)
    assert plant.heads > plant.extra["slots"] >= 10
    per = {}
    for f in got:
        per.setdefault(rp.describe(plant, f[0])[0], []).append(len(f[2].encode("utf-8")))
    seen = [(len(v), sum(v)) for _, v in sorted(per.items())]
    assert seen == plant.extra["regions"]
    for want in ((cap_f, cap_b), (cap_f, cap_b + 1), (cap_f + 1, 12), (1, cap_b), (1, cap_b + 1)):
        assert want in seen[:plant.extra["slots"]], want


@pytest.mark.parametrize("block", rp.STITCH_BLOCKS)
def test_the_host_compiled_core_voids_the_entries_the_stitch_plants_list(block):
    from test_replay_core import RegionOut, load_core, make_params, split_runs
    import stringsext_amd as sx
    plant = rp.stitch(block)
    agree(plant)
    S, n = plant.extra["S"], plant.extra["entries"]
    m = rc.missions(**plant.flags)[0]
    core = load_core()
    runs = split_runs(core, m, plant.data, sxo.runs(m, plant.data, min_chars=2))
    assert [(a, b) for a, b, _ in runs] == [(a, b) for a, b, _, _ in plant.runs] and len(runs) == n
    P, W, _ = make_params(m, plant.data, runs)
    P.max_windows = 512             # (sx_device.hpp kMaxRegionWindowsDefault: a staircase over a block of 128 runs is one region)
    fbuf, abuf = (sx.Finding * 4096)(), (C.c_uint8 * (1 << 20))()
    E, state = 0, []
    for i, (a, b, _) in enumerate(runs):
        want = rp.win_start(a, W)
        if i and want < runs[i - 1][1]:
            state.append("chained")
            continue
        o = RegionOut()
        assert core.sxd_replay_region_host(C.byref(P), i, C.byref(o), fbuf, abuf, 4096, 1 << 20) == 0 and o.status == 0
        state.append("stands" if want >= E else "void")
        if want >= E:
            E = o.end
    assert state.count("stands") + state.count("void") == plant.heads
    void, chained = plant.extra["void"], plant.extra["chained"]
    for what, i in void.items():
        if what != "overrun by the entry region":       # (void only in a chunked scan, by the host's entry region; here: by the run before it)
            assert state[i] == "void" and state[i - 1] != "chained" or what == "behind a chained block", (what, i)
        assert state[i] == "void", (what, i, state[i - 3:i + 2])
    for what, i in chained.items():
        assert state[i] == "chained", (what, i)
    # ... and they lie where the kernels have their edges
    assert void["first of a block"] % S == 0 and void["lane 3"] % S == 3 and void["lane 3"] // S == void["second in a group"] // S
    assert void["two blocks overrun"] % S == 1 and all(s == "void" for s in state[void["two blocks overrun"] - S - 1:void["two blocks overrun"] + 1])
    assert state[void["two blocks overrun"] - S - 2] == "stands" and (void["two blocks overrun"] - S - 1) % S == 0
    assert chained["block begins chained"] % S == 2 and state[chained["block begins chained"] - 4:chained["block begins chained"] + 1] == ["stands"] + ["chained"] * 4
    last = chained["a whole block chained"]
    assert (last + 1) % S == 0 and state[last - S:last + 2] == ["stands"] + ["chained"] * S + ["void"] and void["behind a chained block"] == last + 1
    if S >= 64:
        assert void["lane 63"] % S == 63
    if S > 64:
        assert void["lane 0 of a second group"] % S == 64 and void["two in a row"] % S > 64 and state[void["two in a row"] - 1] == "void"
    for blk in (64, 65) + ((128, 129) if S == 7 else ()):
        assert void["first of block %d" % blk] == blk * S
    assert n > (128 if S == 7 else 64) * S
    if block == 7:
        e = void["overrun by the entry region"]
        assert plant.runs[e - 1][0] // rp.STITCH_CHUNK * rp.STITCH_CHUNK == rp.win_start(plant.runs[e - 1][0], W)    # in a chunk's first window


@pytest.mark.parametrize("one_more", [False, True])
def test_trip_plants_have_one_trips_heads_and_one_more(one_more):
    plant = rp.count_trips(one_more)
    wgs, lanes = rp.count_grid_cap()
    assert plant.heads == len(plant.runs) == wgs * lanes + (1 if one_more else 0) and plant.fast == 0
    q, W = rp.TRIPS_GEOMETRY
    m = rc.missions(**plant.flags)[0]
    runs = sxo.runs(m, plant.data, min_chars=2)
    assert [(a, b) for a, b, _ in runs] == [(a, b) for a, b, _, _ in plant.runs]
    assert all(a - rp.win_start(a, W) == 1 and plant.data[a - 1] == 1 for a, _, _ in runs[:100] + runs[-100:]) and runs[0][0] > 2 * W
    agree(plant)


@pytest.mark.parametrize("shape", sorted(rp.SLAB_CHAIN_SHAPES))
@pytest.mark.parametrize("tail", [False, True])
def test_slab_cuts_fall_on_chained_runs(tail, shape):
    plant = rp.slab_chains(tail, shape)
    agree(plant)
    n, (first, last) = plant.extra["entries"], plant.extra["chain"]
    assert n == len(plant.runs)
    W = 128
    chained = [i > 0 and rp.win_start(plant.runs[i][0], W) < plant.runs[i - 1][1] for i in range(n)]
    assert all(chained[first:last + 1]) and not any(chained[:first]) and not any(chained[last + 1:])
    for slabs in rp.SLABS:
        if n < rp.slab_min_entries(slabs):
            continue
        walked = 0
        for j in range(1, slabs):                  # slab_cuts_kernel
            i = n // slabs * j
            walked += chained[i]
            while i < n and chained[i]:
                i += 1
            assert i <= first - 1 or ((i == last + 1 < n) if tail else (i == n)), (slabs, j, i)
        assert walked > 0, slabs


@pytest.mark.parametrize("slabs", rp.SLABS)
def test_every_plant_replayed_in_slabs_has_entries_for_that_many(slabs):
    """sx_stage_b.cpp slabs_wanted: a list of fewer than 8 entries per slab is replayed as one"""
    assert rp.slab_min_entries(slabs) == 8 * slabs
    plants = rp.slab_plants(slabs)
    assert all(p.extra["entries"] >= 8 * slabs for p in plants)
    assert any("chain" in p.extra for p in plants) and any(any(r[3] for r in p.runs) for p in plants)     # chains and pieces, both
