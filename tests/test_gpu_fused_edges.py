"""The fused scan (stringsext_amd/csrc/sx_fused.hip) at its tile edges, deterministically (run with -m gpu on an MI355X): the planted
atlases of tests/fused_atlas.py — every stretch length around the threshold at every byte offset around a 1 KiB edge, on skipped and
on classified ground, at the fast loop's three trip positions — through sx_device_runs_multi, for every Mission set the kernel is
instantiated for, every prefilter mode, both stream parities and the sub-chunk sizes at which the kernel takes another path; the same
data under the switches that pick the prefilter or the unfused launches; and the small inputs an atlas cannot hold (the end of the
input, the fast loop's first trip, one slot's regions overflowing).  The oracle's sequential decoder is the checker throughout;
test_fused_atlas.py pins the oracle itself on the same atlases."""
import pytest

import fused_atlas as fa
import refconfig as rc
import stringsext_amd as sx
import sxo_binding as sxo
from product_harness import run_cli_product

pytestmark = pytest.mark.gpu

# sub-chunk sizes: every tile is tile 0 | one trip of the fast loop | two trips and a generic tail | long rotations | the default (256 KiB)
SUBCHUNKS = (1024, 4096, 8192, 65536, 0)


def threshold(m):
    return max(1, min(m["chars_min_nb"], m["output_line_char_nb_max"]))


class Device:
    """one buffer in HBM per input, uploaded once and shared by every Scanner of the module (a pointer is good in every context of
    the device); the oracle's runs once per (Mission, input, parity)"""

    def __init__(self):
        self.holder = sx.Scanner(rc.missions(encodings=["utf-8"]), device=0)
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

    def want(self, m, parity):
        sig = (m["encoding"], threshold(m), m["ubf"], m["af"], parity)
        if sig not in self.oracle:
            self.oracle[sig] = sxo.runs(m, self.data, stream_parity=parity, min_chars=threshold(m))
        return self.oracle[sig]

    def close(self):
        self.drop()
        self.holder.close()


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.close()


def check_atlas(dev, ms, key, want_mask, subchunks=SUBCHUNKS):
    """every Mission's runs over the atlas == the oracle's, for every sub-chunk size (a Scanner each) and both parities"""
    at = fa.atlas(key)
    ptr = dev.load(key, at.data)
    mc = [threshold(m) for m in ms]
    for sub in subchunks:
        sc = sx.Scanner(ms, device=0, subchunk_bytes=sub)
        try:
            for parity in (0, 1):
                got = sc.device_runs_multi(list(range(len(ms))), ptr, len(at.data), stream_parity=parity, min_chars=mc)
                assert sc.stats().fused_mask == want_mask, (sub, parity, bin(sc.stats().fused_mask))
                for k, m in enumerate(ms):
                    want = dev.want(m, parity)
                    assert got[k] == want, (key, sub, parity, k, len(got[k]), len(want), fa.first_difference(at, got[k], want))
        finally:
            sc.close()


@pytest.mark.parametrize("set_name,key", fa.ATLAS_CASES, ids=[f"{s}-{k[0]}-n{k[1]}-{k[2]}" for s, k in fa.ATLAS_CASES])
def test_atlas_runs_equal_oracle_runs(dev, set_name, key):
    check_atlas(dev, rc.missions(**fa.set_flags(set_name, key)), key, fa.SET_MASK[set_name])


# The switches sx_switches.hpp keeps for tests, over the same data; a context reads them when it is created.
# SX_FUSED_PREFILTER=0: the kernel without a prefilter (its own instantiations, another occupancy); =2: pairs where groups of four
# would do (thresholds >= 7); SX_FUSED=0: every Mission in its own launch, next to a Mission set that could share one.
SWITCH_CASES = [
    ("SX_FUSED_PREFILTER", "0", "c3", ("u16", 10, "African"), 0b111), ("SX_FUSED_PREFILTER", "0", "c3", ("u16", 3, "African"), 0b111),
    ("SX_FUSED_PREFILTER", "0", "le_be", ("u16", 7, "Greek"), 0b11), ("SX_FUSED_PREFILTER", "0", "c3", ("u8", 13, "Cyrillic"), 0b111),
    ("SX_FUSED_PREFILTER", "2", "c3", ("u16", 7, "African"), 0b111), ("SX_FUSED_PREFILTER", "2", "c3", ("u16", 10, "African"), 0b111),
    ("SX_FUSED_PREFILTER", "2", "le_be", ("u16", 7, "Greek"), 0b11), ("SX_FUSED_PREFILTER", "2", "u8_be", ("u8", 13, "Cyrillic"), 0b11),
    ("SX_FUSED", "0", "c3", ("u16", 10, "African"), 0), ("SX_FUSED", "0", "c3", ("u16", 3, "African"), 0),
    ("SX_FUSED", "0", "c3", ("u8", 12, "Cyrillic"), 0),
]


@pytest.mark.parametrize("name,value,set_name,key,want_mask", SWITCH_CASES,
                         ids=[f"{c[0][3:]}={c[1]}-{c[2]}-{c[3][0]}-n{c[3][1]}-{c[3][2]}" for c in SWITCH_CASES])
def test_atlas_under_the_fused_switches(dev, monkeypatch, name, value, set_name, key, want_mask):
    monkeypatch.setenv(name, value)
    check_atlas(dev, rc.missions(**fa.set_flags(set_name, key)), key, want_mask)


@pytest.mark.parametrize("le_be,mode", fa.MIXED_CASES, ids=[f"le{a}_be{b}" for (a, b), _ in fa.MIXED_CASES])
def test_mixed_thresholds_take_the_weakest_prefilter(dev, le_be, mode):
    """One launch has one prefilter: pairs for thresholds 7 and 4, none for 10 and 2 (Prefilter::mode_for, launch_f) — on the atlas
    of either threshold the Mission of the lower one loses stretches to a prefilter that is too strong."""
    ms = rc.missions(**fa.mixed_flags(*le_be))
    for n in le_be:
        check_atlas(dev, ms, ("u16", n, "African"), 0b11)


END_N = 7


@pytest.mark.parametrize("residue", fa.END_RESIDUES)
def test_the_end_of_the_input(residue):
    """Buffers of 1 to 5 tiles that end `residue` bytes into a tile, the stretch at the very end (its last byte the input's last, or the
    one before, or half a UTF-16 unit left over): the tiles near the end go one at a time with the bytes that exist (n_safe), and with
    1 KiB and 4 KiB sub-chunks the last sub-chunk is a short one behind a full one."""
    ms = rc.missions(**fa.set_flags("c3", ("u16", END_N, "Cyrillic")))
    mc = [threshold(m) for m in ms]
    bufs = fa.end_buffers(residue, END_N)
    want = {(label, k, parity): sxo.runs(m, data, stream_parity=parity, min_chars=mc[k])
            for label, data in bufs for k, m in enumerate(ms) for parity in (0, 1)}
    for sub in (1024, 4096, 0):
        sc = sx.Scanner(ms, device=0, subchunk_bytes=sub)
        try:
            ptr = sc.alloc(5 * fa.TILE)
            for label, data in bufs:
                sc.upload(ptr, data)
                for parity in (0, 1):
                    got = sc.device_runs_multi([0, 1, 2], ptr, len(data), stream_parity=parity, min_chars=mc)
                    assert sc.stats().fused_mask == 0b111
                    for k in range(3):
                        assert got[k] == want[(label, k, parity)], (label, sub, parity, k, got[k], want[(label, k, parity)])
            sc.free(ptr)
        finally:
            sc.close()


@pytest.mark.parametrize("n,flt,top", [(7, "African", None), (3, "African", None), (7, "Greek", None),
                                       (7, "African", 0x07FF), (3, "African", 0x07FF), (7, "Greek", 0x03FF), (3, "Greek", 0x03FF)],
                         ids=lambda v: "letters" if v is None else ("%04X" % v if isinstance(v, int) and v > 99 else str(v)))
def test_a_skipped_tile_in_front_of_the_first_fast_trip(n, flt, top):
    """The input's tile 0 is skipped (nothing forces it), the stretch that begins in it has its aligned group in tile 1: the fast
    loop's first tile, for which no register set holds the tile in front (zprev == false) — the carry word is recomputed from memory.
    With `top`, half the stretch's units are the highest the filter accepts: a prefilter mask one bit short (Prefilter::zero_bits)
    skips their tiles."""
    ms = rc.missions(**fa.set_flags("le_be", ("u16", n, flt)))
    bufs = fa.first_trip_buffers(n, top)
    want = {(label, k, parity): sxo.runs(m, data, stream_parity=parity, min_chars=n)
            for label, data in bufs for k, m in enumerate(ms) for parity in (0, 1)}
    for sub in (4096, 8192, 0):
        sc = sx.Scanner(ms, device=0, subchunk_bytes=sub)
        try:
            ptr = sc.alloc(8 * fa.TILE)
            for label, data in bufs:
                sc.upload(ptr, data)
                for parity in (0, 1):
                    got = sc.device_runs_multi([0, 1], ptr, len(data), stream_parity=parity, min_chars=[n, n])
                    assert sc.stats().fused_mask == 0b11
                    for k in range(2):
                        assert got[k] == want[(label, k, parity)], (label, sub, parity, k, got[k], want[(label, k, parity)])
            sc.free(ptr)
        finally:
            sc.close()


def test_one_slot_overflows_its_regions_the_others_do_not():
    """The UTF-8 Mission has more records in one sub-chunk than its region holds (64), the UTF-16 Missions a few: whichever launch ends
    up producing a Mission's runs — the fused one, or the re-scan of the Mission that overflowed — they are the oracle's."""
    n = 10
    ms = rc.missions(**fa.set_flags("c3", ("u16", n, "African")))
    at = fa.atlas(("u16", n, "African"))
    data = bytearray(at.data[:3 * 256 * 1024])
    for i in range(200):                                    # 200 UTF-8 strings in the second sub-chunk, 100 of them two-byte characters
        s = (("string%04d-" % i) * 2).encode() if i % 2 else ("שלום-" * 3).encode()
        at_byte = 256 * 1024 + 3000 + i * 700
        data[at_byte:at_byte + len(s)] = s
    data = bytes(data)
    want = [[sxo.runs(m, data, stream_parity=parity, min_chars=n) for m in ms] for parity in (0, 1)]
    assert sum(1 for r in want[0][0] if r[0] // (256 * 1024) == 1) > 64 and all(len(want[0][k]) < 200 for k in (1, 2))
    sc = sx.Scanner(ms, device=0)
    try:
        ptr = sc.alloc(len(data))
        sc.upload(ptr, data)
        rescans = 0
        for _ in range(2):           # (the second round starts from what the first learnt about the UTF-8 Mission's density)
            for parity in (0, 1):
                got = sc.device_runs_multi([0, 1, 2], ptr, len(data), stream_parity=parity, min_chars=[n] * 3)
                rescans = max(rescans, sc.stats().rescans)
                for k in range(3):
                    assert got[k] == want[parity][k], (parity, k, len(got[k]), len(want[parity][k]), fa.first_difference(at, got[k], want[parity][k]))
        assert rescans >= 1          # (the overflow did happen)
        sc.free(ptr)
    finally:
        sc.close()


@pytest.mark.parametrize("key", [("u16", 2, "African"), ("u16", 3, "African"), ("u16", 10, "African"), ("u8", 12, "Cyrillic")],
                         ids=["none", "pairs", "fours", "utf8"])
def test_atlas_end_to_end_equals_oracle(key):
    """stage B sees no difference: the whole scan of an atlas per prefilter mode prints what the oracle prints"""
    ms = rc.missions(**fa.set_flags("c3", key))
    data = fa.atlas(key).data
    assert run_cli_product(ms, [data], radix="x", device=0) == sxo.run_cli(ms, [data], radix="x")
