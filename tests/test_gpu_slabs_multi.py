"""A busy Mission next to quiet ones, replayed in slabs (csrc/sx_stage_b.cpp device_replay_mission): `-e utf-8 -e utf-16le -e utf-16be
-u African` on the planted buffers of tests/slab_plant.py (what they hold: tests/test_slab_plant.py, on the CPU).  The UTF-8
Mission's findings reach the host as one block per slab, the last one while the other Missions are collected and replayed on the
host; merge_findings interleaves the blocks with the other Missions' findings and starts a segment where the UTF-8 Mission enters
its next block.  Every case is compared with the oracle finding by finding, and must really have taken the slabs: as many segments
as slabs, cut where the planted buffer says (with SX_SLABS=1: one segment per buffer)."""
import pytest

import refconfig as rc
import slab_plant as sp
import stringsext_amd as sx
import sxo_binding as sxo

pytestmark = pytest.mark.gpu
SLICE = 4096
_oracle = {}


def oracle_findings(flavour):
    """the reference's merged list for the whole buffer: slice by slice, position, then mission; computed once per buffer (the
    Missions' states run on across scan calls and pieces, so chunking does not change it)"""
    if flavour not in _oracle:
        ms = rc.missions(**sp.FLAGS)
        data = sp.plant(flavour).data
        scanners = [sxo.Scanner(m) for m in ms]
        out = []
        for off in range(0, len(data), SLICE):
            here = []
            for k, s in enumerate(scanners):
                here += [(f["position"], k, f["precision"], f["completes"], f["s"]) for f in s.scan(data[off:off + SLICE], file_id=1)]
            here.sort(key=lambda t: (t[0], t[1]))
            out += [(pos, ms[k]["mission_id"], prec, comp, text) for pos, k, prec, comp, text in here]
        text = sxo.run_cli(ms, [data], radix="x")
        assert len(out) == text.count(b"\n") - 1 > 12000      # (the two ways through the oracle agree on how many there are)
        _oracle[flavour] = out
    return _oracle[flavour]


def scan(flavour, monkeypatch, env, chunks=1):
    """(findings as the oracle lists them, per scan call: [findings per segment])"""
    for name in ("SX_SLABS", "SX_PIECE_MIB", "SX_DEFER_MIN_BYTES"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SX_DEVICE_JOIN_MIN", "1")     # the run list stays on the device whatever its length
    monkeypatch.setenv("SX_WAVE_REPLAY", "0")         # the lane-per-region replay, whatever the density
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    data = sp.plant(flavour).data
    step = len(data) // chunks
    sc = sx.Scanner(rc.missions(**sp.FLAGS), device=0)     # (the switches are read here)
    got, shape = [], []
    try:
        for off in range(0, len(data), step):
            res = sc.scan(data[off:off + step], file_id=1)
            shape.append([n for _, n, _ in res.segments()])
            got += [(f["position"], f["mission_id"], f["precision"], f["completes"], f["s"]) for f in res.findings()]
            res.free()
    finally:
        sc.close()
    return got, shape


def first_utf8_positions(got, shape):
    """position of the first UTF-8 finding of every segment"""
    utf8_id = rc.missions(**sp.FLAGS)[0]["mission_id"]
    out, at = [], 0
    for segs in shape:
        for n in segs:
            out.append(next(f[0] for f in got[at:at + n] if f[1] == utf8_id))
            at += n
    return out


def planted_text(flavour, kind, start):
    p = sp.plant(flavour)
    lo, hi, _ = next(r for r in getattr(p, kind) if r[0] == start)
    return p.data[lo:hi].decode({"utf8": "utf-8", "utf16le": "utf-16-le", "utf16be": "utf-16-be"}[kind])


def check_cuts(flavour, got, shape, bounds):
    """every segment but a buffer's first begins where the planted buffer puts the cut: at a block start"""
    firsts = first_utf8_positions(got, shape)
    sizes = [n for segs in shape for n in segs]
    later = [i for i, is_first in enumerate(i == 0 for segs in shape for i in range(len(segs))) if not is_first]
    assert len(later) == len(bounds)
    for i, block in zip(later, bounds):
        base, p, at = block * sp.BLOCK, firsts[i], sum(sizes[:i])
        if flavour == "u16":
            assert p == base + 40, (p, base)
            # the other Missions' strings around and at the cut are the findings next to the segment's first one
            around = [f[4] for f in got[at - 8:at + 8]]
            for kind, start in (("utf16be", base - 20), ("utf16le", base), ("utf16be", base + 18)):
                assert planted_text(flavour, kind, start) in around, (kind, start)
        else:
            assert p in (base - 20, base, base + 128, base + 256), (p, base)    # a piece of the stretch that is open across it


@pytest.mark.parametrize("flavour", ["u16", "long"])
@pytest.mark.parametrize("slabs", [2, 3, 4])
def test_slabs_next_to_quiet_missions_agree_with_the_oracle(flavour, slabs, monkeypatch):
    want = oracle_findings(flavour)
    got, shape = scan(flavour, monkeypatch, {"SX_SLABS": str(slabs)})
    assert got == want
    assert len(shape[0]) == slabs, shape
    check_cuts(flavour, got, shape, [sp.BLOCKS // slabs * j for j in range(1, slabs)])


def test_one_slab_is_one_segment(monkeypatch):
    got, shape = scan("u16", monkeypatch, {"SX_SLABS": "1"})
    assert got == oracle_findings("u16") and [len(s) for s in shape] == [1]


@pytest.mark.parametrize("flavour", ["u16", "long"])
def test_two_scan_calls_each_in_slabs(flavour, monkeypatch):
    """the second call's first slab has the host's exact entry part in front of it ("long": a stretch is open across the calls)"""
    got, shape = scan(flavour, monkeypatch, {"SX_SLABS": "3"}, chunks=2)
    assert got == oracle_findings(flavour)
    assert [len(s) for s in shape] == [3, 3], shape
    check_cuts(flavour, got, shape, [2, 4, 8, 10])


@pytest.mark.parametrize("flavour", ["u16", "long"])
def test_two_pieces_each_in_slabs(flavour, monkeypatch):
    got, shape = scan(flavour, monkeypatch, {"SX_SLABS": "3", "SX_PIECE_MIB": "3"})
    assert got == oracle_findings(flavour)
    assert [len(s) for s in shape] == [6], shape
    firsts = first_utf8_positions(got, shape)
    assert [(p + 20) // sp.BLOCK for p in (firsts[1], firsts[2], firsts[4], firsts[5])] == [2, 4, 8, 10]   # ("long": from 20 bytes in front of the block on)
    assert firsts[3] // sp.BLOCK in (5, 6)                                                                   # the second piece


def test_an_output_at_the_deferral_threshold_takes_the_whole_list_path(monkeypatch):
    """SX_DEFER_MIN_BYTES below what the UTF-8 Mission writes: the slab that would take the sum there hands the Mission back, its
    findings wait in HBM as one list and reach the host as they do without slabs — one segment, the same findings"""
    env = {"SX_DEFER_MIN_BYTES": "65536"}
    one, shape_one = scan("u16", monkeypatch, dict(env, SX_SLABS="1"))
    got, shape = scan("u16", monkeypatch, dict(env, SX_SLABS="3"))
    assert got == one == oracle_findings("u16")
    assert shape == shape_one and [len(s) for s in shape] == [1]
