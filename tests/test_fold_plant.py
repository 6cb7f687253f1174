"""What tests/fold_plant.py promises of its lines, asserted on the oracle's strings (no GPU): a line is a finding, the lines hold every
kind of character the fold treats differently, and the fold decides what neither the byte comparison nor the ASCII fold decides.
These are checks of the plant that tests/test_gpu_fold_device.py stands on; the fold they judge it by is the library's on the host,
sx_fold_utf8 (stringsext_amd.fold), which has to agree with fold_plant.fold(), the rule in Python, on every string they look at."""
import numpy as np

import fold_plant as fp
import long_plant as lp
import result_plant as rp
import stringsext_amd as sx

N = 3000


def test_a_line_is_a_finding_at_the_counts_the_gpu_tests_take():
    for n in (1, 63, 64, 65, 129, N):
        rows = rp.expected(fp.ms1(), fp.buffer(n))
        assert rows.strs == fp.lines(n), n
        assert [sx.fold(x) for x in rows.strs] == [fp.fold(x) for x in rows.strs], n          # the plant's oracle and the library agree on it
    assert all(4 <= len(x.decode()) <= 60 for x in fp.lines(N))
    assert rp.expected(fp.ms2(), fp.buffer(N)).n > N                 # two Missions: the ASCII one finds the runs of four and more


def test_the_lines_hold_what_they_are_meant_to():
    strs = rp.expected(fp.ms1(), fp.buffer(N)).strs
    text = b"\n".join(strs).decode()
    for ch in ("P", "Å", "Σ", "ς", "П", "Ꮳ", "ꮃ", "\U00010400", "\u023A", "\u023E", "\u212A", "\u1E9E", "ß", "\u0130", "漢", "\u00B5", "\u2126"):
        assert ch in text, hex(ord(ch))
    folded = [sx.fold(s) for s in strs]
    assert folded == [fp.fold(s) for s in strs]
    assert sum(len(f) > len(s) for f, s in zip(folded, strs)) > 50 and sum(len(f) < len(s) for f, s in zip(folded, strs)) > 50
    assert sum(f == s for f, s in zip(folded, strs)) > 10             # some lines the fold leaves alone
    # the fold joins classes that the bytes and the ASCII fold keep apart
    assert len(set(folded)) < len({s.lower() for s in strs}) - 100 < len(set(strs)) - 100
    assert max(folded.count(f) for f in set(folded[:400])) >= 3
    # bytes >= 0x80 at the first and at the last byte of an 8-byte word, wherever a string lies: back to back, every alignment occurs
    at, first, last = 0, 0, 0
    for s in strs:
        first += any(b >= 0x80 and (at + i) % 8 == 0 for i, b in enumerate(s))
        last += any(b >= 0x80 and (at + i) % 8 == 7 for i, b in enumerate(s))
        at += len(s)
    assert first > N // 4 and last > N // 4
    # grep -i: every needle stands in lines in more than one spelling
    for needle in fp.NEEDLES:
        f = fp.fold(needle.encode())
        held = {s for s, g in zip(strs, folded) if f in g}
        assert len(held) > len({s for s in held if needle.encode() in s}) > 0, needle


def test_the_host_fold_agrees_with_the_rule_on_every_line():
    for s in fp.lines(N):
        assert sx.fold(s) == fp.fold(s), s


# ---- the lines of tests/test_gpu_fold_edges.py

def test_the_page_lines_hold_every_page_of_the_table_and_what_lies_next_to_it():
    pages, pts, lines = fp.pages(), fp.page_points(), fp.page_lines()
    assert len(pages) == 35 and pages[0] == 0 and len(pts) == 4394 and len(set(pts)) == 4392
    assert [hex(p << 7) for p in pages[32:]] == ["0x11880", "0x16e00", "0x1e900"]       # what fold_load copies in its loop's second trip
    strs = rp.expected(fp.ms1(), lp.buffer(lines)).strs
    assert strs == lines and len(lines) == 96                                         # every line is found whole
    assert all(len(x.decode()) <= 60 for x in lines) and sum(x.startswith(b"fill") for x in lines) == 96 - 92
    held = set(b"".join(strs).decode())
    assert not [hex(c) for c in pts if chr(c) not in held]
    for k, p in enumerate(pages):
        on = [c for c in range(max(p << 7, 0x80), (p + 1) << 7) if chr(c) in held]
        assert len(on) == (128 if p else 0), k
        assert p == 0 or any(fp.fold_char(chr(c)) != chr(c) for c in on), k               # ... a wrong page base shows
        for c in ((p << 7) - 1, (p + 1) << 7):                                          # the neighbours on no page: kFoldNoPage
            assert c < 0x80 or c >> 7 in pages or (chr(c) in held and fp.fold_char(chr(c)) == chr(c)), hex(c)
    limit = (pages[-1] + 1) << 7
    assert limit == 0x1E980 and sum(c >= limit for c in set(pts)) == 5 and {limit - 1, limit, 0x10FFFF} <= {ord(x) for x in held}
    assert [sx.fold(x) for x in strs] == [fp.fold(x) for x in strs]
    assert 0 < sum(fp.fold(x) == x for x in strs) - 4 < 92                      # some lines stay as they are, besides the filler


def test_the_split_lines_are_cut_in_every_way_a_character_can_be():
    six = {(2, 1), (3, 1), (3, 2), (4, 1), (4, 2), (4, 3)}
    assert set(fp.SPLIT_CUTS.values()) == six
    merged = rp.expected(fp.ms2v(), fp.split_buffer()).strs
    one = rp.expected(fp.ms1(), lp.buffer(fp.split_lines())).strs
    assert one == fp.split_lines() and all(x in merged for x in fp.split_lines())
    for strs in (merged, one):
        found, cuts = fp.split_pairs(strs)
        assert set(cuts) == six and min(cuts.values()) >= 2, cuts
        # one lone lead byte, one lone continuation byte, and the last match of all ends in a lead byte
        assert b"\xc8" in found and b"\xba" in found and found[-1] == b"EN8\xd0" and strs[-1] == fp.SPLIT_LAST.encode()
        assert any(fp.fold(x) != x for x in found) and all(found)
    # what a lane that read on would make of a left half: the character, folded
    assert fp.fold(b"ABC\xd0") + fp.fold(b"\x96DEF") == b"abc\xd0\x96def" != fp.fold("ABCЖDEF".encode())
    assert fp.cut_of(b"ABC\xd0", b"\x96DEF") == (2, 1) and fp.cut_of(b"A3\xe2\x84", b"\xaaB") == (3, 2) and fp.cut_of(b"ABC", b"DEF") is None
    assert [sx.fold(x) for x in found] == [fp.fold(x) for x in found]
    # (how the GPU tests ask the host twin: every string in ONE call, a \n between them — no sequence goes on across it)
    assert sx.fold(b"\n".join(found)).replace(b"\n", b"") == b"".join(fp.fold(x) for x in found) != fp.fold(b"".join(found))


def test_the_long_lines_are_found_whole():
    for q, ms in ((255, lp.msl1()), (1024, fp.msl())):
        lines = fp.long_lines(q)
        rows = rp.expected(ms, lp.buffer(lines))
        utf8 = [s for s, m in zip(rows.strs, rows.mission) if m == len(ms) - 1]
        assert utf8 == lines, q
        folded = {len(s): len(fp.fold(s)) for s in lines}
        assert (folded[2 * q], folded[3 * q], folded[4 * q]) == (3 * q, q, 4 * q)
        reps = {255: 30, 1024: 120}[q]
        for j in range(9):      # j characters that grow, 8-byte words of ASCII, one character that shrinks
            assert folded[2 * j + 8 * reps + 3] == 3 * j + 8 * reps + 1
            assert ("\u023A" * j + "ABCDEFGH" * reps + "\u212A").encode() in lines
        assert max(len(x.decode()) for x in lines) == q
        # the words of ASCII go out by every store, whatever the first string's place: a result's strings lie back to back
        folded = [fp.fold(x) for x in rows.strs]
        for base in range(8):
            stores = fp.word_stores(rows.strs, fp.back_to_back(rows.strs), fp.back_to_back(folded) + base)
            assert min(stores) > 0, (q, base, stores)


def test_the_limit_lines_are_found_whole_and_a_folded_length_passes_32768():
    lines = fp.limit_lines()
    rows = rp.expected(lp.limit_ms(), lp.buffer(lines))
    assert [s for s, m in zip(rows.strs, rows.mission) if m == 1] == lines and rows.n == 20
    lengths = sorted((len(s), len(fp.fold(s))) for s in lines if len(s) >= 16000)
    assert lengths == [(16000, 16000), (16001, 16002), (32000, 48000), (48000, 16000), (64000, 64000)]
    assert max(len(fp.fold(s)) for s in rows.strs) == 64000 < 0xFFFF and sum(len(fp.fold(s)) > 1 << 15 for s in rows.strs) == 2
    big = next(s for s in lines if len(s) == 64000)
    assert sum(a != b for a, b in zip(big, fp.fold(big))) == 16000                    # every character of it changes
    assert all(sx.fold(s) == fp.fold(s) for s in rows.strs)
    stores = fp.word_stores(rows.strs, fp.back_to_back(rows.strs), fp.back_to_back([fp.fold(s) for s in rows.strs]))
    assert min(stores) >= 1000, stores                     # merged records: back to back, and both arenas begin on a multiple of 8
