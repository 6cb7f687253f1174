"""The planted buffers of tests/slab_plant.py hold what they claim (no GPU needed): for each of the three Missions the oracle's runs
are exactly the planted stretches — none missing, none extra —, every block of a buffer holds the same number of them, and what the
GPU tests look for around a slab cut lies at every block start."""
import pytest

import refconfig as rc
import slab_plant as sp
import sxo_binding as sxo


@pytest.mark.parametrize("flavour", ["u16", "long"])
def test_the_oracle_finds_exactly_what_was_planted(flavour):
    p = sp.plant(flavour)
    assert len(p.data) == sp.BLOCKS * sp.BLOCK
    ms = rc.missions(**sp.FLAGS)
    assert [m["encoding"] for m in ms] == [m["encoding"] for m in rc.missions(encodings=["utf-8", "utf-16le", "utf-16be"])]
    for m, planted in zip(ms, (p.utf8, p.utf16le, p.utf16be)):
        assert len(planted) >= sp.BLOCKS
        assert sxo.runs(m, p.data, stream_parity=0, min_chars=sp.N) == planted
    # the busy Mission is busy enough for the device (4096 runs, also in each half), the others are not
    assert len(p.utf8) >= 2 * 4096 and len(p.utf16le) < 4096 and len(p.utf16be) < 4096
    per_block = [sum(1 for r in p.utf8 if r[0] // sp.BLOCK == b) for b in range(sp.BLOCKS)]
    assert len(set(per_block[1:-1])) == 1 and abs(per_block[0] - per_block[1]) <= 1 and abs(per_block[-1] - per_block[1]) <= 1
    text = sxo.run_cli(ms, [p.data], radix="x")
    for letter in b"abc":
        assert b"(%c " % letter in text


def test_what_lies_at_the_block_starts():
    u16, long_ = sp.plant("u16"), sp.plant("long")
    for b in range(1, sp.BLOCKS):
        base = b * sp.BLOCK
        assert any(r[0] == base for r in u16.utf16le)                               # a finding exactly at the cut
        assert any(r[0] == base + 18 for r in u16.utf16be)                          # a few bytes behind it
        assert any(base - 20 == r[0] and r[1] <= base - 4 for r in u16.utf16be)     # a few bytes in front of it
        assert any(r[0] == base + 40 for r in u16.utf8)                             # the run the list is cut at
        assert any(r[0] == base - 20 and r[1] == base + 280 for r in long_.utf8)    # open across the cut, longer than a window
