"""What tests/measure_plant.py promises of its lines, asserted on the oracle's strings (no GPU): the sources of
tests/test_gpu_measure_device.py really hold strings on both sides of 255 bytes, a count above 255, wide strings in the runs and at the
places the kernels' edges need, every class bit a Mission lets through, and multi-byte characters.  The words they are judged by are
measure_plant.measure()'s, the rule in Python; the library on the host, sx_measure_bytes (stringsext_amd.measure), has to agree with
it on every string they look at.

SX_MEASURE_CONTROL: no Mission here finds a control byte inside a string — a control byte ends a finding —, so that bit is pinned on
the host only (tests/test_measure_core.py, every single byte)."""
import numpy as np
import pytest

import fold_plant as fp
import long_plant as lp
import measure_plant as mp
import result_plant as rp
import stringsext_amd as sx


def runs(flags):
    """the lengths of the runs of True"""
    edges = np.diff(np.concatenate([[0], np.asarray(flags, dtype=np.int8), [0]]))
    return (np.nonzero(edges == -1)[0] - np.nonzero(edges == 1)[0]).tolist()


def classes_of(strs):
    bits = 0
    for s in set(strs):
        bits |= mp.measure(s)
    return {name for bit, name in mp.CLASS_NAMES.items() if bits & bit}


def agree(strs):
    for s in set(strs):
        assert sx.measure(s) == mp.measure(s), s[:60]


def test_the_edge_lines_under_two_missions():
    lines = mp.edge_lines()
    rows = rp.expected(lp.msl2(), lp.buffer(lines))
    assert rows.n == 2 * len(lines) and sorted(rows.strs) == sorted(lines + lines)            # every line whole, once per Mission
    agree(rows.strs)
    length = rows.length.astype(np.int64)
    assert {254, 255, 256, 257, 600} <= set(length.tolist())
    wide = length > mp.NARROW_MAX
    # parts of 1024 findings: two parts' worth of narrow records in front, two parts' worth of wide ones in a row, a run longer than
    # a wavefront, and wide records at every place of a wavefront wherever the parts begin (a period of 3 against 64)
    assert int(np.argmax(wide)) >= 2 * 1024 and max(runs(wide)) >= 2 * 1024 and sum(1 for r in runs(wide) if 64 < r < 1024) >= 1
    alone = [i for i in range(1, rows.n - 1) if wide[i] and not wide[i - 1] and not wide[i + 1]]
    assert {i % 64 for i in alone} == set(range(64)) and {i % 3 for i in alone[:60]} == {alone[0] % 3}
    # a count above 255 with entropy 0, every printable value, and a narrow string of q directly behind a wide one of nothing else
    assert mp.measure(mp.SEVENS) == mp.DIGIT | 1 << mp.DISTINCT_SHIFT | 600 << mp.CHARS_SHIFT and rows.strs.count(mp.SEVENS) == 2
    w = mp.measure(mp.PRINTABLE)
    assert (w >> mp.DISTINCT_SHIFT) & 0x1FF == 95 and w & (mp.LOWER | mp.UPPER | mp.DIGIT | mp.SPACE | mp.PUNCT) == w & (0x7F << 25) and len(mp.PRINTABLE) > 255
    assert rows.strs.count(mp.PRINTABLE) == 2
    behind = [i for i in range(rows.n - 1) if rows.strs[i] == b"q" * 400 and rows.strs[i + 1] == mp.LEFTOVER]
    assert len(behind) == 2
    assert classes_of(rows.strs) == {"lower", "upper", "digit", "space", "punct"}


def test_the_edge_lines_of_the_lane_per_region_replay():
    lines = mp.one_edge_lines()
    rows = rp.expected(lp.msl1(), lp.buffer(lines))
    assert rows.strs == lines
    agree(rows.strs)
    assert [len(x) for x in lines[:4]] == list(mp.EDGE_LENGTHS) and [mp.measure(x) >> 32 for x in lines[:4]] == [254, 255, 255, 254]
    length = rows.length.astype(np.int64)
    assert (length > 255).sum() >= 20 and int(length.max()) > 900
    assert any(len(a) > 255 and b == mp.LEFTOVER for a, b in zip(lines, lines[1:]))                   # narrow behind wide
    assert classes_of(rows.strs) == {"lower", "upper", "digit", "space", "punct", "high"}
    assert sum(mp.measure(s) >> 32 < len(s) for s in lines) > 30                                   # chars against bytes


def test_the_limit_lines_hold_16000_and_64000_bytes():
    rows = rp.expected(lp.limit_ms(), lp.buffer(lp.limit_lines()))
    assert {16000, 64000} <= set(rows.length.tolist())
    agree(rows.strs)
    big = [s for s in rows.strs if len(s) == 64000]
    assert big and all(mp.measure(s) >> 32 == 16000 and mp.measure(s) & mp.HIGH for s in big)
    assert any(max(s.count(bytes([b])) for b in set(s)) > 65535 // 4 for s in big)                    # counts far above a byte's, and a halfword's quarter


def test_the_second_trip_lines_and_the_scripts():
    for r in (64, 1000):
        lines = mp.second_trip_lines(r)
        rows = rp.expected(fp.ms1(), lp.buffer(lines))
        assert rows.strs == lines and sorted(lines[-1]) == sorted(lines[0] + b"!")
    agree(rows.strs)
    assert classes_of(rows.strs) == {"lower", "upper", "digit", "space", "punct", "high"}
    words = [mp.measure(s) for s in rows.strs]
    assert sum(w >> 32 < len(s) for w, s in zip(words, rows.strs)) > 500 and sum(not w & mp.HIGH for w in words) > 20
    # the fields spread: entropy and chars decide something
    assert len({w & 0xFFFF for w in words}) > 200 and len({w >> 32 for w in words}) > 40


# ---- the lines of tests/test_gpu_measure_edges.py

QUIET, TWO_WINDOWS = b"\x80", 2 * 4096      # (the wave path's padding, as tests/test_gpu_fold_edges.py make_from() adds it)
W_DEVICE = 256 * 4 * 8                      # measure_wide_kernel's wavefronts on 256 CUs; the GPU test reads its own from the device


@pytest.mark.parametrize("w", [24, W_DEVICE])
def test_the_wide_trip_lines_list_more_than_two_strings_a_wavefront(w):
    lines = mp.wide_trip_lines(w)
    rows = rp.expected(lp.msl2(), lp.buffer(lines))
    assert rows.n == 2 * len(lines) and sorted(rows.strs) == sorted(lines + lines)            # every line whole, once per Mission
    agree(rows.strs)
    length = rows.length.astype(np.int64)
    wide = length > mp.NARROW_MAX
    assert int(wide.sum()) == 2 * w + 4 >= 2 * w + 3 and 0 < int((~wide).sum()) and 256 <= int(length[wide].min()) and int(length[wide].max()) <= 330
    assert len({x for x in rows.strs if len(x) > mp.NARROW_MAX}) == w + 2                         # no wide line twice
    kinds = [[mp.trip_line(k) for k in range(kind, 16 * mp.TRIP_KINDS, mp.TRIP_KINDS)] for kind in range(mp.TRIP_KINDS)]
    assert all(x in rows.strs for kind in kinds for x in kind[:w // mp.TRIP_KINDS])
    assert [classes_of(kind) for kind in kinds[:2]] == [{"digit"}, {"lower"}] and classes_of(kinds[2]) >= {"lower", "digit", "space", "punct"}
    assert all((mp.measure(x) >> mp.DISTINCT_SHIFT) & 0x1FF <= 7 for x in kinds[3])               # one byte and a number
    # a wavefront that did not clear: the histogram of a + b (of a + a' + b, the third string of a wavefront) taken for b's
    for ka in kinds:
        for kb in kinds:
            for i, a in enumerate(ka):
                for b in kb:
                    assert mp.uncleared(a, b) != mp.measure(b) and mp.uncleared(a + ka[i - 1], b) != mp.measure(b), (a[:20], b[:20])
    assert mp.uncleared(b"", kinds[2][0]) == mp.measure(kinds[2][0])                              # (the model is the rule where nothing is left)


@pytest.mark.parametrize("r", [64, 1000])
def test_the_late_wide_lines_and_the_neighbours_at_255_bytes(r):
    lines = mp.late_wide_lines(r)
    data = lp.buffer(lines)
    rows = rp.expected(lp.msw(), data + QUIET * max(0, TWO_WINDOWS - len(data)))
    assert rows.strs == lines and rows.n == r + mp.LATE_TAIL
    agree(rows.strs)
    wide = np.nonzero(rows.length.astype(np.int64) > mp.NARROW_MAX)[0].tolist()
    assert wide == [0] + [r + p for p in mp.LATE_WIDE] and mp.LATE_WIDE == (0, 1, 63, 64) and mp.LATE_TAIL == 65
    assert len({rows.strs[i] for i in wide}) == len(wide)
    # 64 characters on both sides of 255 bytes, next to each other
    assert rows.strs[:2] == [mp.SMALLEST_WIDE, mp.LARGEST_NARROW] and [len(x) for x in rows.strs[:2]] == [256, 255]
    assert [mp.measure(x) >> mp.CHARS_SHIFT for x in rows.strs[:2]] == [64, 64] and mp.LARGEST_NARROW[:252] == mp.SMALLEST_WIDE[:252]
    assert all(mp.measure(rows.strs[i]) >> mp.CHARS_SHIFT == 64 and mp.measure(rows.strs[i]) & mp.HIGH for i in wide)


def test_the_word_edge_lines_cover_every_word_count_and_every_pair_of_ends():
    lines = mp.word_edge_lines()
    rows = rp.expected(lp.msl2(), lp.buffer(lines))
    assert rows.n == 2 * len(lines) and sorted(rows.strs) == sorted(lines + lines)
    agree(rows.strs)
    length = rows.length.astype(np.int64)
    head = (np.cumsum(length) - length) % 8                                   # one segment, strings back to back from an aligned place
    mp.word_edges_complete(head.tolist(), length.tolist())
    counts, _, _, _ = mp.word_edges(head.tolist(), length.tolist())
    # (lane 63 has the last word of 64, lane 0 the first and the last of 65 and of 129, lane 62 the last of 63 and of 127)
    assert {w: sorted(h for v, h in counts if v == w) for w in (64, 65)} == {64: list(range(8)), 65: list(range(8))}
    assert 1024 in length.tolist() and not any(w > 129 for w, _ in counts)


def test_the_reset_lines_put_a_part_without_wide_strings_behind_one_of_nothing_else():
    lines = mp.reset_lines()
    data = lp.buffer(lines)
    rows = rp.expected(lp.msl2(), data)
    assert rows.n == 2 * len(lines) and sorted(rows.strs) == sorted(lines + lines)
    agree(rows.strs)
    sizes = mp.merge_parts(rows.position.tolist(), int(rows.length.sum()), len(data))
    assert sum(sizes) == rows.n and max(sizes) <= 2 * 1024
    wide, at, pattern = rows.length.astype(np.int64) > mp.NARROW_MAX, 0, ""
    for n in sizes:
        part = wide[at:at + n]
        pattern += "w" if part.all() else "n" if not part.any() else "m"
        at += n
    assert pattern == "wwwwwwwwnn", (pattern, sizes)
    assert int(wide.sum()) > 2 * 1024 and int((~wide).sum()) > 2 * 1024
