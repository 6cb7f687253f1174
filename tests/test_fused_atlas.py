"""The planted inputs of tests/fused_atlas.py hold what they claim (no GPU needed): on every atlas the GPU tests of the fused scan use
(test_gpu_fused_edges.py), the oracle's runs for a stretch's own Mission are exactly the planted stretches of at least n characters —
none missing, none extra —, every event kind lies at all three trip positions of the fast loop, and no sub-chunk holds so many runs
that a fused launch would be abandoned for the overflow re-scan."""
import pytest

import fused_atlas as fa
import refconfig as rc
import sxo_binding as sxo

KEYS = sorted({key for _, key in fa.ATLAS_CASES} | {("u16", 4, "African")})
kSubchunk = 256 * 1024     # the default sub-chunk (sx_stage_a.cpp subchunk_bytes)
kHalfRegion = 32           # half of the 64 record slots a sub-chunk's region has (sx_ctx.hpp region_cap)


def most_runs_per_subchunk(runs):
    count = {}
    for start, _, _ in runs:
        count[start // kSubchunk] = count.get(start // kSubchunk, 0) + 1
    return max(count.values(), default=0)


def mission_sets_on(key):
    sets = [rc.missions(**fa.set_flags(s, k)) for s, k in fa.ATLAS_CASES if k == key]
    if key[0] == "u16" and key[2] == "African":
        sets += [rc.missions(**fa.mixed_flags(le, be)) for (le, be), _ in fa.MIXED_CASES if key[1] in (le, be)]
    return sets


@pytest.mark.parametrize("key", KEYS, ids=lambda k: "-".join(map(str, k)))
def test_the_oracle_finds_exactly_the_planted_stretches(key):
    kind, n, flt = key
    at = fa.atlas(key)
    assert len(at.planted) == len(at.events) == len(at.data) // (at.spacing * fa.TILE) and len(at.data) % fa.TILE == 0
    assert all(b[0] - a[1] >= 4 * fa.TILE - 200 for a, b in zip(at.planted, at.planted[1:]))       # events cannot touch
    own = ["utf-16le", "utf-16be"] if kind == "u16" else ["utf-8"]
    for enc in own:
        m = rc.missions(encodings=[enc], chars_min=str(n), unicode_block_filter=flt)[0]
        for parity in (0, 1):
            want = fa.expected(at, enc, n, parity)
            assert len(want) >= len(at.events) // 5          # (the atlas is not vacuous)
            got = sxo.runs(m, at.data, stream_parity=parity, min_chars=n)
            assert got == want, (enc, parity, fa.first_difference(at, got, want))
    # every kind of event at the fast loop's three trip positions
    where = {}
    for ev in at.events:
        where.setdefault((ev.enc, ev.chars, ev.off, ev.bg), set()).add(ev.edge_tile % 3)
    kinds = {(enc, chars, off, bg) for enc in (fa.UTF16 if kind == "u16" else fa.UTF8) for chars in fa.lengths(n) for off in fa.offsets(n)
             for bg in range(3)}
    assert set(where) == kinds and all(v == {0, 1, 2} for v in where.values())
    # the fused launch is never abandoned: at most half a region's records per default sub-chunk, for every Mission of every set
    seen = set()
    for ms in mission_sets_on(key):
        for m in ms:
            mc = max(1, min(m["chars_min_nb"], m["output_line_char_nb_max"]))
            sig = (m["encoding"], mc, m["ubf"], m["af"])
            if sig in seen:
                continue
            seen.add(sig)
            for parity in (0, 1):
                most = most_runs_per_subchunk(sxo.runs(m, at.data, stream_parity=parity, min_chars=mc))
                assert most <= kHalfRegion, (sig, parity, most)


@pytest.mark.parametrize("n", [11, 12, 13, 14, 15])
def test_the_utf8_atlas_holds_the_edges_the_candidate_test_depends_on(n):
    """a two-byte character split by the tile edge and by the edge of the tile's last lane (16 bytes in front of it); stretches
    open over 11, 12, 13 and 14 bytes where the tile ends: both sides of the fast loop's candidate test of at most 12 bytes"""
    at = fa.atlas(("u8", n, "Cyrillic"))
    split_edge = split_lane = False
    open_over = set()
    for ev in at.events:
        edge = ev.edge_tile * fa.TILE
        for cut, name in ((edge, "edge"), (edge - 16, "lane")):
            if ev.start < cut < ev.end and at.data[cut] & 0xC0 == 0x80:      # a continuation byte right behind the cut
                if name == "edge": split_edge = True
                else: split_lane = True
        if ev.start < edge < ev.end and ev.chars >= n:
            open_over.add(edge - ev.start)
    assert split_edge and split_lane and {11, 12, 13, 14} <= open_over


def test_the_small_buffers_end_as_they_say():
    n = 7
    sizes = set()
    for residue in fa.END_RESIDUES:
        for label, data in fa.end_buffers(residue, n):
            assert len(data) % fa.TILE == residue and 1 <= -(-len(data) // fa.TILE) <= 5, label
            sizes.add(len(data))
    assert len(sizes) == 5 * len(fa.END_RESIDUES)
    # a full stretch at the very end is what its own Mission reports last (threshold 1: whatever is left of a clipped stretch counts)
    for label, data in fa.end_buffers(33, n):
        enc, how = label.split("/")[2:]
        m = rc.missions(encodings=[fa.mission_name(enc)], chars_min="1", unicode_block_filter="Cyrillic")[0]
        ends = {r[1] for parity in (0, 1) for r in sxo.runs(m, data, stream_parity=parity, min_chars=1)}
        assert (len(data) - (0 if how == "last" else 1)) in ends, label
    for label, data in fa.first_trip_buffers(n):
        assert len(data) == 8 * fa.TILE and data[:fa.TILE - 64] == b"\xff" * (fa.TILE - 64), label
        assert data[fa.TILE - 1] != 0xFF and data[fa.TILE] != 0xFF, label      # the stretch begins in tile 0 and goes on in tile 1
