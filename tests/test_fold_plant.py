"""What tests/fold_plant.py promises of its lines, asserted on the oracle's strings (no GPU): a line is a finding, the lines hold every
kind of character the fold treats differently, and the fold decides what neither the byte comparison nor the ASCII fold decides.
These are checks of the plant that tests/test_gpu_fold_device.py stands on; the fold they judge it by is the library's on the host,
sx_fold_utf8 (stringsext_amd.fold), which has to agree with fold_plant.fold(), the rule in Python, on every string they look at."""
import fold_plant as fp
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
