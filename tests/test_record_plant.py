"""The planted inputs of tests/record_plant.py against the oracle, on the CPU: the runs every stage A plant says it planted are the
oracle's runs, its record counts per region follow from them by the model of a record, and every interleave plant that relies on the
merger's way to the host has the findings that way asks for.  tests/test_gpu_record_paths.py and tests/test_gpu_interleave_edges.py run
the same plants through the library."""
import os
import re

import pytest

import fused_atlas as fa
import record_plant as rp
import refconfig as rc
import result_plant
import sxo_binding as sxo

MISSIONS = {"ascii": (rp.ASCII_FLAGS, False), "fused": (rp.FUSED_FLAGS, True)}


def mission(name):
    flags, two_byte = MISSIONS[name]
    return rc.missions(**flags)[0], two_byte


def check(plant, m, what):
    """the plant's runs are ALL the stretches the oracle sees (min_chars = 1), and for every threshold those that are long enough"""
    got = sxo.runs(m, plant.data, min_chars=1)
    assert got == plant.runs, (what, len(got), len(plant.runs), rp.first_difference(plant, got, plant.runs))
    for n in rp.JOIN_THRESHOLDS:
        assert sxo.runs(m, plant.data, min_chars=n) == rp.kept(plant.runs, n), (what, n)


def test_the_constants_are_where_the_plants_look_for_them():
    assert rp.constant("kScanPerBlock") == 1024 and rp.constant("kPackLanes") == 16 and rp.constant("kMergeLists") == 16
    assert rp.constant("kRecBlock") == 16 and rp.sum_scan_trip() == 256 and rp.default_region_cap() == 64
    assert rp.FUSED_FLAGS == fa.set_flags("u8", ("u8", 4, "Cyrillic"))
    lanes, cap = rp.constant("kPackLanes"), rp.default_region_cap()
    assert rp.count_cycle() == (0, 1, 2, lanes - 1, lanes, lanes + 1, 31, 32, 33, 47, 48, 49, cap - 1, cap)


@pytest.mark.parametrize("name", list(MISSIONS))
def test_counts_plants(name):
    m, two = mission(name)
    per, cap = rp.constant("kScanPerBlock"), rp.default_region_cap()
    for n_regions in rp.counts_sizes():
        for raised in (None,) if n_regions != per + 1 else (None, 0, n_regions - 2):
            plant, counts = rp.counts_plant(n_regions, two, raised)
            check(plant, m, ("counts", n_regions, raised))
            assert (n_regions - 1) * rp.SUB < len(plant.data) < n_regions * rp.SUB
            assert rp.records_per_region(plant.runs, len(plant.data), 4) == counts
            assert n_regions < len(rp.count_cycle()) or set(counts) - {cap + 1} == set(rp.count_cycle())
            assert [c for c in counts if c > cap] == ([] if raised is None else [cap + 1]) and (raised is None or counts[raised] == cap + 1)
            # several strings inside one lane's 16 bytes: the next string begins 5 to 8 (7 to 11) bytes behind
            gaps = {b[0] - a[0] for a, b in zip(plant.runs, plant.runs[1:]) if a[0] // rp.SUB == b[0] // rp.SUB}
            assert gaps <= (set(range(7, 12)) if two else set(range(5, 9))) and (n_regions < len(rp.count_cycle()) or len(gaps) >= 3)
            assert not two or any(e - s != c for s, e, c in plant.runs) or not plant.runs
    sparse = rp.sparse_plant(per + 1, two)
    check(sparse, m, "sparse")
    assert 4 * len(sparse.runs) < (per + 1) * 2     # below a quarter of the slots of regions of 2 .. 64


@pytest.mark.parametrize("ending", rp.JOIN_ENDINGS)
@pytest.mark.parametrize("name", list(MISSIONS))
def test_join_plants(name, ending):
    m, two = mission(name)
    plant = rp.join_plant(two, ending)
    check(plant, m, ("join", ending))
    data, runs, cap = plant.data, plant.runs, rp.default_region_cap()
    assert (900 << 10) < len(data) < (1300 << 10)
    assert runs[0][0] == 0 and runs[-1][1] == len(data) and (len(data) % rp.SUB == 0) == (ending == "multiple")
    for n in rp.JOIN_THRESHOLDS:
        counts = rp.records_per_region(runs, len(data), n)
        assert max(counts) <= cap - 1 and max(counts) > 2 and sum(counts) > 1024 + 256      # regions hold it; regions of 2 do not; a pool of 1024 grows
        # the threshold cases: i + (n - 1 - i) dropped, i + (n - i) kept, for every i
        over = [(s, e, c) for s, e, c in runs if s // rp.SUB != (e - 1) // rp.SUB]
        width = 2 if two else 1
        for i in range(1, n):
            for total in (n - 1, n):
                assert any(c == total and e - s == total * width and (-s) % rp.SUB == i * width for s, e, c in (over if i <= total - 1 else runs)), (n, i, total)
    # what test_gpu_record_paths.py's rescans under SX_REGION_CAP=2 rest on: on either side of "a run to two regions", with a margin
    n_regions = (len(data) + rp.SUB - 1) // rp.SUB
    assert len(rp.kept(runs, 4)) > n_regions and len(rp.kept(runs, 7)) * 100 < n_regions * 46, (n_regions, len(rp.kept(runs, 4)), len(rp.kept(runs, 7)))
    spans = sorted((e - 1) // rp.SUB - s // rp.SUB - 1 for s, e, c in runs if (e - 1) // rp.SUB - s // rp.SUB >= 2)
    assert [k for k in spans if k in rp.JOIN_CHAINS] == sorted(rp.JOIN_CHAINS) or ending == "chain_tail"
    assert set(rp.JOIN_CHAINS) <= set(spans)
    # touching but not continuing: a stretch ends with an edge's last byte and the next begins one byte behind the edge; and the mirror image
    ends, starts = {e for _, e, _ in runs}, {s for s, _, _ in runs}
    assert any(e % rp.SUB == 0 and e + 1 in starts for e in ends) and any(s % rp.SUB == 0 and s - 1 in ends for s in starts)
    if two:
        assert any(data[k * rp.SUB - 1] >= 0xC0 for k in range(1, len(data) // rp.SUB))       # a lead byte as an edge's last byte
        assert any(e - s != c for s, e, c in runs)
    last = runs[-1]
    if ending == "lone": assert last[0] // rp.SUB == (last[1] - 1) // rp.SUB and last[2] >= 4
    if ending == "chain_tail": assert last[0] // rp.SUB + 2 <= (last[1] - 1) // rp.SUB
    if ending == "open_short": assert last[2] == 3 and last[0] // rp.SUB != (last[1] - 1) // rp.SUB


def test_second_trip_plant():
    m, _ = mission("ascii")
    plant, counts = rp.second_trip_plant()
    trip = rp.sum_scan_trip() * rp.constant("kScanPerBlock")
    n_regions = (len(plant.data) + rp.SUB - 1) // rp.SUB
    assert n_regions == trip + 5 and len(plant.data) % rp.SUB
    got = sxo.runs(m, plant.data, min_chars=4)
    assert got == plant.runs, rp.first_difference(plant, got, plant.runs)
    model = rp.records_per_region(plant.runs, len(plant.data), 4)
    assert {w: c for w, c in enumerate(model) if c} == counts
    assert [counts[w] for w in (trip - 1, trip, trip + 1, n_regions - 1)] == [3, rp.default_region_cap(), 2, 1]
    assert all(c == 1 for w, c in counts.items() if w not in (trip - 1, trip, trip + 1)) and all(w in counts for w in range(0, n_regions, 61))


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("name", list(MISSIONS))
def test_key_width_plants(name, dense):
    m, two = mission(name)
    for length in rp.key_width_lengths():
        plant = rp.key_width_plant(length, dense, two)
        assert len(plant.data) == length
        check(plant, m, ("key_width", length, dense))
        assert plant.runs[0][0] == 0 and plant.runs[-1][:2] == (length - (8 if two else 4), length) and plant.runs[-1][2] == 4
        j = 0
        while (1 << j) < length - 32:
            assert any(s < (1 << j) < e for s, e, _ in plant.runs), j
            j += 1
        assert j >= 16
        assert (max(rp.records_per_region(plant.runs, length, 4)) > 2 + 32) == dense
        # what test_gpu_record_paths.py's rescans rest on: with regions of 2 slots the dense plant lies well on one side of "a run to
        # two regions" — three runs to four regions and more around 2^16, one run to eight regions and fewer around 2^20
        n_regions, n_runs = (length + rp.SUB - 1) // rp.SUB, len(rp.kept(plant.runs, 4))
        if dense:
            assert n_runs * 4 >= n_regions * 3 if length < (1 << 17) else n_runs * 8 <= n_regions, (length, n_runs, n_regions)


def test_sx_timing_only_prints():
    """the tests read the path from SX_TIMING's lines: the switch must do nothing else"""
    uses = []
    for name in sorted(os.listdir(rp.CSRC)):
        if name.endswith((".cpp", ".hip", ".hpp")) and name not in ("sx_switches.cpp", "sx_switches.hpp"):
            src = rp._source(name)
            for m in re.finditer(r"sw\.timing\b(?!2)", src):
                assert src[:m.start()].endswith("if (ctx->") and src[m.end()] == ")", (name, src[m.start() - 20:m.end() + 20])
                rest = src[m.end() + 1:].lstrip()
                if rest.startswith("{"):        # a block: locals and the line, no HIP call, no way out
                    rest = rest[1:rest.index("\n    }")]
                    assert "hip" not in rest and "return" not in rest and "ctx->stats" not in rest, (name, rest)
                    rest = rest[rest.index("fprintf("):]
                uses.append((name, rest[:14]))
    assert len(uses) >= 3 and all(rest == "fprintf(stderr" for _, rest in uses), uses


# ---- interleave ----

def findings_per_mission(flags, data):
    ms = rc.missions(encodings=flags)
    rows = result_plant.expected(ms, data)
    return [int((rows.mission == k).sum()) for k in range(len(ms))], rows


@pytest.mark.parametrize("name", list(rp.interleave_plants()))
def test_interleave_plants(name):
    p = rp.interleave_plants()[name]
    per, rows = findings_per_mission(p.flags, p.data)
    assert 3 <= len(p.flags) <= 5 or name == "small_parts"
    if p.host_way:
        assert sum(per) >= 4096 and sum(1 for n in per if n) >= 2, per
    # the same flags: the same findings; different flags: disjoint lists
    for a in range(len(p.flags)):
        for b in range(a + 1, len(p.flags)):
            sa, sb = [rows.raw[i].split(b"\t")[::2] for i in range(rows.n) if rows.mission[i] == a], [rows.raw[i].split(b"\t")[::2] for i in range(rows.n) if rows.mission[i] == b]
            if p.flags[a] == p.flags[b]:
                assert sa == sb          # (position and string)
            else:
                assert not {x[1] for x in sa} & {x[1] for x in sb}
    if name.startswith("twins"): assert all(per) and all(p.flags.count(f) == 2 for f in p.flags if f != rp.mission_flag("ascii"))
    if name.startswith("empty"): assert per.count(0) == 1 and per[int(name[-1])] == 0
    if name == "apart":
        span = [(int(rows.position[rows.mission == k].min()), int(rows.position[rows.mission == k].max())) for k in range(4)]
        assert all(span[2][1] < span[k][0] for k in (0, 1, 3)) and all(span[0][0] > span[k][1] for k in (1, 2, 3))
    if name.startswith("one_tile"):
        big = p.flags.index(rp.mission_flag("ascii"))
        lone = p.flags.index(rp.mission_flag("Greek"))
        pos = rows.position[rows.mission == big]
        span = int(rows.position.max() - rows.position.min())
        assert per[lone] == 1 and per[big] >= 4096 and (int(pos.max()) - int(pos.min())) * (sum(per) // 64) < span      # inside one of sum / 64 tiles
    if name == "parts":
        at_slices = set(range(0, len(p.data), rp.SLICE))
        assert at_slices <= set(rows.position[rows.mission == 0].tolist()) and list(rows.position[rows.mission == 0]) == list(rows.position[rows.mission == 3])
        inside = rows.position[rows.mission == 1]
        assert len({int(x) // rp.SLICE for x in inside}) == 1 and int(rows.position[rows.mission == 2].max()) < 2 * rp.SLICE


@pytest.mark.parametrize("total", rp.INTERLEAVE_TOTALS)
def test_interleave_totals(total):
    """what the merger sees is `total` findings: all four lists together, the twin's among them"""
    assert rp.INTERLEAVE_TOTALS == (1, 63, 64, 65, 129)
    p = rp.interleave_plants()["total%d" % total]
    per, rows = findings_per_mission(p.flags, p.data)
    assert len(per) == 4 and sum(per) == total and rows.n == total and not p.host_way
    assert per[0] == per[3] == total // 4 and (total == 1 or all(per))       # (the first and the last Mission are twins)


@pytest.mark.parametrize("n", [17, 18, 26])
def test_many_missions(n):
    flags = rp.many_missions(n)
    assert len(flags) == n and rp.constant("kMergeLists") == 16
    per, rows = findings_per_mission(flags, rp.many_plant())
    assert sum(per) >= 4096 and per.count(0) == (0 if n == 17 else 1) and (n == 17 or per[-1] == 0)
    assert flags[0] == flags[16] and flags[15] != flags[16] and per[0] == per[16] > 0       # ties on either side of the 16th
    assert list(rows.position[rows.mission == 0]) == list(rows.position[rows.mission == 16])


@pytest.mark.parametrize("residue", rp.COPY_RESIDUES)
def test_copy_plants(residue):
    flags = [rp.mission_flag("ascii"), rp.mission_flag("Cyrillic")]
    per, rows = findings_per_mission(flags, rp.copy_plant(residue))
    bytes_16 = 16 * sum(per) + int(rows.length.sum())       # the part as 16-byte records and their strings
    assert min(per) >= 33000 and bytes_16 >= (1 << 20) and bytes_16 % 16 == residue and (32 * sum(per) + int(rows.length.sum())) % 16 == residue
