"""Stage A's record paths (stringsext_amd/csrc/sx_sort.hip, sx_stage_a.cpp) on planted inputs (run with -m gpu on an MI355X): the pack
of the per-sub-chunk regions (region_block_scan_kernel, region_sum_scan_kernel, region_pack_kernel), the large regions and the pool
(region_invalidate_kernel, split_records_kernel, the radix sort, join_records_kernel) and the join into runs (RecIsHead,
accumulate_runs_kernel, scatter_long_runs_kernel), through Scanner.device_runs / device_runs_multi with 1 KiB sub-chunks.  The plants
are tests/record_plant.py's (test_record_plant.py pins them on the oracle): they are made of strings any classifier finds; what they
aim at is where records land and how many there are.  Every comparison is exact equality with the oracle's runs, and every call
asserts the path it took from the lines SX_TIMING writes, stats().rescans and, for the fused Mission, stats().fused_mask."""
import pytest

import record_plant as rp
import refconfig as rc
import stringsext_amd as sx
import sxo_binding as sxo

pytestmark = pytest.mark.gpu

MISSIONS = {"ascii": (rp.ASCII_FLAGS, False), "fused": (rp.FUSED_FLAGS, True)}
JOINS = {"device": "1", "host": str(1 << 30)}          # SX_DEVICE_JOIN_MIN: from one record on | above any record count
REGIONS, LARGE, POOL = "records (regions)", "record slots (large regions)", "record slots (pool)"


class Device:
    """one buffer in HBM per input, uploaded once and shared by every Scanner of the module; the oracle's runs once per
    (Mission, input, threshold)"""

    def __init__(self):
        self.holder = sx.Scanner(rc.missions(encodings=["ascii"]), device=0)
        self.key, self.ptr, self.data = None, None, b""
        self.oracle = {}

    def load(self, key, data):
        if key != self.key:
            self.drop()
            self.ptr = self.holder.alloc(max(len(data), 1))
            self.holder.upload(self.ptr, data)
            self.key, self.data = key, data
        return self.ptr

    def drop(self):
        if self.ptr is not None:
            self.holder.free(self.ptr)
        self.key, self.ptr, self.data = None, None, b""
        self.oracle.clear()

    def want(self, m, n):
        sig = (m["encoding"], m["ubf"], m["af"], n)
        if sig not in self.oracle:
            self.oracle[sig] = sxo.runs(m, self.data, min_chars=n)
        return self.oracle[sig]

    def close(self):
        self.drop()
        self.holder.close()


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.close()


class Case:
    """one Scanner (a context reads the SX_* switches when it is created) with SX_TIMING on; call() checks one device_runs call"""

    def __init__(self, monkeypatch, capfd, dev, mission, join, env=(), **options):
        flags, self.two = MISSIONS[mission]
        self.ms = rc.missions(**flags)
        self.fused, self.join, self.dev, self.capfd = mission == "fused", join, dev, capfd
        monkeypatch.setenv("SX_TIMING", "1")
        monkeypatch.setenv("SX_DEVICE_JOIN_MIN", JOINS[join])
        for name, value in env:
            monkeypatch.setenv(name, value)
        self.sc = sx.Scanner(self.ms, device=0, subchunk_bytes=rp.SUB, **options)

    def call(self, key, plant, n, path, rescans, fused=None, what=""):
        """the runs of `plant` at threshold n == the oracle's; the record path, the join and the rescans are the expected ones"""
        ptr = self.dev.load(key, plant.data)
        self.capfd.readouterr()
        got = self.sc.device_runs(0, ptr, len(plant.data), min_chars=n)
        err = self.capfd.readouterr().err
        want = self.dev.want(self.ms[0], n)
        where = (key, n, self.join, path, what)
        assert got == want, (where, len(got), len(want), rp.first_difference(plant, got, want))
        lines = rp.stage_a_lines(err)
        assert len(lines) == 1 and lines[0][0] == 0, (where, err)
        line = lines[0][1]
        assert path in line and sum(p in line for p in (REGIONS, LARGE, POOL)) == 1, (where, line)
        n_records = int(line.split(" ms, ")[1].split(" ")[0])
        if self.join == "device" and n_records:
            assert ("device pack+join" if path == REGIONS else "device sort+join") in line and "d2h runs" in line, (where, line)
        else:
            assert ", d2h " in line and "host join" in line and "device" not in line, (where, line)
        st = self.sc.stats()
        assert st.rescans == rescans, (where, st.rescans, rescans)       # (a call's statistics begin at zero)
        if self.fused:      # (the fused launch takes a Mission whose records go to regions; the pool's Mission has its own launch)
            assert st.fused_mask == ((path != POOL) if fused is None else fused), (where, st.fused_mask)
        else:
            assert st.fused_mask == 0
        return line

    def close(self):
        self.sc.close()


# ---- 1. counts ----

@pytest.mark.parametrize("join", list(JOINS))
@pytest.mark.parametrize("mission", list(MISSIONS))
def test_counts_every_region_edge(monkeypatch, capfd, dev, mission, join):
    """c(w) records per region through 0, 1, 2, the pack lanes' count - 1 / + 0 / + 1 (a lane's second trip), 31 .. 33, 47 .. 49, cap - 1
    and cap (a full region overflows nothing), several strings inside one lane's 16 bytes (rank inside a region), at region counts
    around region_block_scan_kernel's block (block_off at region 1024 and 1025) up to four blocks and three regions"""
    case = Case(monkeypatch, capfd, dev, mission, join)
    try:
        for n_regions in rp.counts_sizes():
            plant, counts = rp.counts_plant(n_regions, case.two)
            line = case.call(("counts", case.two, n_regions, None), plant, 4, REGIONS, 0)
            assert " %d records (regions)" % sum(counts) in line, (n_regions, sum(counts), line)
    finally:
        case.close()


@pytest.mark.parametrize("no_large", [False, True], ids=["large", "pool"])
@pytest.mark.parametrize("raised", ["first", "last_full", "behind_a_full_one"])
@pytest.mark.parametrize("join", list(JOINS))
@pytest.mark.parametrize("mission", list(MISSIONS))
def test_counts_one_region_over(monkeypatch, capfd, dev, mission, join, raised, no_large):
    """one region holds cap + 1 records next to regions that hold cap: the scan is repeated once, with larger regions or (SX_NO_LARGE_REGIONS)
    into the pool; a second call starts from what the first learnt; a sparse buffer brings the regions back, the dense one overflows again"""
    n_regions = rp.constant("kScanPerBlock") + 1
    case = Case(monkeypatch, capfd, dev, mission, join, env=[("SX_NO_LARGE_REGIONS", "1")] if no_large else [])
    try:
        at = dict(first=0, last_full=n_regions - 2, behind_a_full_one=len(rp.count_cycle()))[raised]
        dense, counts = rp.counts_plant(n_regions, case.two, at)
        assert counts[at] == rp.default_region_cap() + 1 and (raised != "behind_a_full_one" or counts[at - 1] == rp.default_region_cap())
        sparse = rp.sparse_plant(n_regions, case.two)
        path = POOL if no_large else LARGE
        case.call(("counts", case.two, n_regions, at), dense, 4, path, 1, fused=True, what="first")       # (the fused launch came first)
        case.call(("counts", case.two, n_regions, at), dense, 4, path, 0, what="learnt")
        case.call(("sparse", case.two, n_regions), sparse, 4, path, 0, what="sparse")
        case.call(("counts", case.two, n_regions, at), dense, 4, path, 1, fused=True, what="dense again")
    finally:
        case.close()


# ---- 2. join ----

ONCE = {(4, 0): 1}          # the rescans of (threshold, call), for every ending; ONCE: the Scanner's very first call only
JOIN_PATHS = {
    "regions": ([], {}, REGIONS, {}),
    "pool": ([("SX_REGION_CAP", "0")], {}, POOL, {}),
    "pool_grows": ([("SX_REGION_CAP", "0")], dict(record_capacity=1024), POOL, ONCE),
    # the plant has more runs of 4 characters than regions, and fewer runs of 7 than a runs-to-regions ratio of 0.46 (test_record_plant.py):
    # the large regions stay behind the calls at 4 and behind the first at 7, whose few runs bring the regions of 2 back — they overflow
    # in the second call at 7 and, its runs few again, in the next ending's first at 4
    "large": ([("SX_REGION_CAP", "2")], {}, LARGE, {(4, 0): 1, (4, 1): 0, (7, 0): 0, (7, 1): 1}),
    "small_then_pool": ([("SX_REGION_CAP", "2"), ("SX_NO_LARGE_REGIONS", "1")], {}, POOL, ONCE),
}


@pytest.mark.parametrize("path", list(JOIN_PATHS))
@pytest.mark.parametrize("join", list(JOINS))
@pytest.mark.parametrize("mission", list(MISSIONS))
def test_join_edges(monkeypatch, capfd, dev, mission, join, path):
    """threshold splits over an edge (dropped one character short, kept at the threshold), neighbours that touch without continuing,
    chains over 1 .. 600 sub-chunks (the join kernels' blocks, `chars` summed by atomics), a first record open at its start, four
    endings; under every record path, both joins, thresholds 4 and 7, two calls per Scanner"""
    env, options, words, rescans = JOIN_PATHS[path]
    case = Case(monkeypatch, capfd, dev, mission, join, env=env, **options)
    assert rp.constant("kRecBlock") == 16
    try:
        assert rp.JOIN_THRESHOLDS == (4, 7)
        for k, ending in enumerate(rp.JOIN_ENDINGS):
            plant = rp.join_plant(case.two, ending)
            for n in rp.JOIN_THRESHOLDS:
                for call in (0, 1):
                    again = rescans.get((n, call), 0) if k == 0 or rescans is not ONCE else 0
                    took_fused = True if again and path in ("large", "small_then_pool") else None     # (the fused launch came first)
                    case.call(("join", case.two, ending), plant, n, words, again, fused=took_fused, what=(ending, call))
    finally:
        case.close()


def test_join_three_fused_missions(monkeypatch, capfd, dev):
    """the pack and the join once per slot of the fused launch: three Missions over the two-byte variant"""
    import fused_atlas as fa
    monkeypatch.setenv("SX_TIMING", "1")
    monkeypatch.setenv("SX_DEVICE_JOIN_MIN", "1")
    ms = rc.missions(**fa.set_flags("c3", ("u8", 4, "Cyrillic")))
    plant = rp.join_plant(True, "chain_tail")
    ptr = dev.load(("join", True, "chain_tail"), plant.data)
    sc = sx.Scanner(ms, device=0, subchunk_bytes=rp.SUB)
    try:
        for parity in (0, 1):
            capfd.readouterr()
            got = sc.device_runs_multi([0, 1, 2], ptr, len(plant.data), stream_parity=parity, min_chars=[4, 4, 4])
            lines = rp.stage_a_lines(capfd.readouterr().err)
            assert sc.stats().fused_mask == 0b111 and sc.stats().rescans == 0
            assert sorted(k for k, _ in lines) == [0, 1, 2] and all(REGIONS in line for _, line in lines), lines
            for k, m in enumerate(ms):
                want = sxo.runs(m, plant.data, stream_parity=parity, min_chars=4)
                assert got[k] == want, (parity, k, len(got[k]), len(want), rp.first_difference(plant, got[k], want))
            assert len(got[0]) > 1000 and "device pack+join" in dict(lines)[0]
    finally:
        sc.close()


# ---- 3. the second trip of region_sum_scan_kernel ----

def test_second_trip_of_the_block_sum_scan(monkeypatch, capfd, dev):
    """256 x kScanPerBlock + 5 regions: the block sums of the last five take the loop's second trip, and the carry decides where every
    record behind it lands — regions of 3, cap and 2 records around the trip's end, both joins"""
    plant, counts = rp.second_trip_plant()
    assert len(plant.data) > rp.sum_scan_trip() * rp.constant("kScanPerBlock") * rp.SUB
    try:
        for join in JOINS:
            case = Case(monkeypatch, capfd, dev, "ascii", join)
            try:
                line = case.call(("second_trip",), plant, 4, REGIONS, 0)
                assert " %d records (regions)" % sum(counts.values()) in line, line
            finally:
                case.close()
    finally:
        dev.drop()


# ---- 4. the sort's key width ----

@pytest.mark.parametrize("cap", ["0", "2"])
@pytest.mark.parametrize("mission", list(MISSIONS))
def test_sort_key_width(monkeypatch, capfd, dev, mission, cap):
    """len around 2^16 and 2^20: end_bit follows from len; runs at 0, at every power of two and at the input's end; with regions of 2
    that overflow, the large regions' unused slots (the pool's unused slots of a block of kRecBlock) must still sort last"""
    case = Case(monkeypatch, capfd, dev, mission, "device", env=[("SX_REGION_CAP", cap)])
    try:
        # SX_REGION_CAP=2: the first call overflows; around 2^16 the plant has three runs to four regions and more (test_record_plant.py)
        # and the large regions stay, around 2^20 it has one run to eight regions and fewer: each call brings the regions of 2 back
        # and the next one overflows again
        assert len(rp.key_width_lengths()) == 6
        for length, rescans in zip(rp.key_width_lengths(), (1, 0, 0, 0, 1, 1) if cap == "2" else (0,) * 6):
            plant = rp.key_width_plant(length, cap == "2", case.two)
            line = case.call(("key_width", case.two, cap, length), plant, 4, POOL if cap == "0" else LARGE, rescans)
            slots = int(line.split(" ms, ")[1].split(" ")[0])
            assert slots > sum(rp.records_per_region(plant.runs, length, 4)), line       # (there are unused slots)
    finally:
        case.close()
