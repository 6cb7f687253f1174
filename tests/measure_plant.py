"""The rule of sx_result_measure_device and sx_measure_bytes restated in Python as include/stringsext_amd.h states it — lg16() and
measure(), the oracle of every word in the tests (tests/test_measure_core.py on the CPU, tests/test_gpu_measure_device.py on the
device) —, and the planted lines that put strings at the edges of the two kernels: a LANE measures a string of at most 255 bytes with
one-byte counters, a WAVEFRONT a longer one.  Everything is a function of a line's place: no random state.  Expected findings come
from the oracle alone (result_plant.expected()); tests/test_measure_plant.py asserts on its strings what the lines are planted for."""
import bisect
import collections
import math

import fold_plant as fp
import long_plant as lp
import result_plant as rp

ENTROPY_SHIFT, DISTINCT_SHIFT, CHARS_SHIFT = 0, 16, 32
LOWER, UPPER, DIGIT, SPACE, PUNCT, CONTROL, HIGH = (1 << k for k in range(25, 32))
CLASS_NAMES = {LOWER: "lower", UPPER: "upper", DIGIT: "digit", SPACE: "space", PUNCT: "punct", CONTROL: "control", HIGH: "high"}
NARROW_MAX = 255                # the longest string a lane measures


def lg16(x):
    """LG(x), 1 <= x < 2^32: log2(x) in units of 2^-16 by sixteen squarings of the mantissa"""
    assert 1 <= x < 1 << 32
    e = x.bit_length() - 1
    m, f = x << (31 - e), 0
    for _ in range(16):
        m = (m * m) >> 31
        f <<= 1
        if m >= 1 << 32:
            f |= 1
            m >>= 1
    return e << 16 | f


def byte_class(b):
    if 0x61 <= b <= 0x7A:
        return LOWER
    if 0x41 <= b <= 0x5A:
        return UPPER
    if 0x30 <= b <= 0x39:
        return DIGIT
    if b in (0x20, 0x09):
        return SPACE
    if 0x21 <= b <= 0x7E:
        return PUNCT
    return HIGH if b >= 0x80 else CONTROL


_lg, _words = {}, {}
_CLASS = [byte_class(b) for b in range(256)]


def measure(s):
    """the word of the byte string s (remembered per string: the sources repeat their lines)"""
    if s in _words:
        return _words[s]
    n = len(s)
    if n == 0:
        return 0
    count = collections.Counter(s)                                   # {byte: how often}
    for c in {n} | set(count.values()):
        if c not in _lg:
            _lg[c] = lg16(c)
    t = n * _lg[n] - sum(c * _lg[c] for c in count.values())
    assert t >= 0
    chars = n - sum(c for b, c in count.items() if 0x80 <= b <= 0xBF)
    word = min(65535, t // (16 * n)) | len(count) << DISTINCT_SHIFT | chars << CHARS_SHIFT
    for b in count:
        word |= _CLASS[b]
    _words[s] = word
    return word


def entropy(s):
    """Shannon entropy of the bytes of s in bits per byte, in floating point"""
    n = len(s)
    count = [0] * 256
    for b in s:
        count[b] += 1
    return math.fsum(-c / n * math.log2(c / n) for c in count if c) if n else 0.0


def info(strs):
    """sx_measure_info of a result with these strings, from the words"""
    words = [measure(s) for s in strs]
    return dict(findings=len(strs), bytes=sum(len(s) for s in strs), chars=sum(w >> CHARS_SHIFT for w in words),
                wide=sum(1 for s in strs if len(s) > NARROW_MAX), ascii=sum(1 for w in words if not w & HIGH))


# ---- the planted lines

SEVENS = b"7" * 600                                              # one count above 255, entropy 0
PRINTABLE = bytes(range(0x20, 0x7F)) * 3                         # 285 bytes: wide, every printable value three times
EDGE_LENGTHS = (254, 255, 256, 257)
# A narrow line of q behind a wide line full of q.  The two kernels count in counters of their own — a lane's one-byte block, a
# wavefront's 256 words —, so nothing can leak from the wide line into this one: what the line pins is a narrow lane's word for a
# string of one dominant letter, and that the neighbour's being wide does not disturb it.  The narrow lane's own clearing is pinned
# where a lane takes a second record (second_trip_lines()), the wide wavefront's by wide_trip_lines()
# (tests/test_gpu_measure_edges.py)
LEFTOVER = b"leftover? no: " + b"q" * 20


def ascii_edge(n):
    """an ASCII line of n bytes"""
    return b"%03d:" % n + lp.text(n, n - 4)


def wide(k):
    """a wide ASCII line, 256 to 300 bytes, a function of k"""
    return b"w%05d " % k + lp.text(7000 + k, 249 + rp.mix(k) % 45)


WIDE_RUN, ALL_WIDE, NO_WIDE = 200, 1100, 1200


def edge_lines():
    """for long_plant.msl2() under SX_MERGE_PART_FINDINGS=1024 — every line is found by both Missions, and the merged records go
    window by window, a window's lines once per Mission —: NO_WIDE short lines (parts without a wide string); a mixed stretch of one
    wide line and two narrow ones in turn, a period of 3 records against the wavefront's 64, so that a wide record stands at every
    place of a wavefront, the first and the last among them, and a narrow record directly behind a wide one; the lines of
    EDGE_LENGTHS, SEVENS, PRINTABLE, and LEFTOVER behind a wide line full of its letter (which no counter connects: see LEFTOVER); WIDE_RUN wide lines in a row: wherever a part ends among
    them, more records in a row than a wavefront has lanes; ALL_WIDE wide lines: more than two parts' worth of records, so one part holds nothing else"""
    out = rp.lines(NO_WIDE)
    for k in range(150):
        out += [wide(k), rp.lines(NO_WIDE)[k + 3], rp.lines(NO_WIDE)[k + 700]]
    out += [ascii_edge(n) for n in EDGE_LENGTHS] + [SEVENS, b"between", PRINTABLE, b"q" * 400, LEFTOVER, b"7" * 256, b"77777", b"7" * 255]
    out += [wide(1000 + k) for k in range(WIDE_RUN)] + rp.lines(NO_WIDE)[100:140]
    out += [wide(2000 + k) for k in range(ALL_WIDE)] + [b"edge last line"]
    return out


E = "é".encode()


def one_edge_lines():
    """for long_plant.msl1(), `-q 255`, the lane-per-region replay (unpacked records): the lines of 255 characters at most among the
    above — 254 and 255 bytes of ASCII, then 256 and 257 bytes in 255 and 254 characters —, a line of 255 times one digit, and
    long_plant.one_lines(), whose lines of four-byte characters are wide"""
    own = [ascii_edge(254), ascii_edge(255), ascii_edge(253)[:253] + E + b"!", ascii_edge(251)[:251] + E * 3, b"7" * 255, LEFTOVER, b"q" * 130 + E * 64, LEFTOVER]
    assert [len(x) for x in own[:4]] == list(EDGE_LENGTHS) and all(len(x.decode()) <= 255 for x in own)
    return lp.fitted(own + lp.one_lines(), 255)


def second_trip_lines(r):
    """for fold_plant.ms1() on the wave path: r lines of fold_plant, then line 0 with one byte more — record r is the one record of the
    narrow kernel's second trip and falls to the lane that had record 0: its bytes are that string's plus one"""
    out = fp.lines(r)
    last = out[0] + b"!"
    assert 4 <= len(last.decode()) <= 60 and len(last) <= fp.Q
    return out + [last]


# ---- the lines of tests/test_gpu_measure_edges.py: what only runs above W strings, behind R records, and at the wide lanes' word edges

def uncleared(a, b):
    """what a wavefront of measure_wide_kernel would say of b if it still had a's counts: the histogram of a + b under b's length,
    characters and classes.  T of measure_finish is unsigned: below zero it wraps, and the entropy field saturates"""
    count = collections.Counter(a + b)
    n = len(b)
    t = n * lg16(n) - sum(c * lg16(c) for c in count.values())
    ent = 65535 if t < 0 else min(65535, t // (16 * n))
    return ent | len(count) << DISTINCT_SHIFT | measure(b) >> 25 << 25


TRIP_KINDS = 4                  # the alphabets of trip_line(), by k % 4
TRIP_NARROW = 7                 # a narrow line behind every seventh wide one


def trip_line(k):
    """wide line k of wide_trip_lines(): 256 to 330 bytes; digits only, lower case only, text, or one byte repeated behind a number"""
    n, kind = 256 + rp.mix(k) % 75, k % TRIP_KINDS
    if kind == 0:
        x = b"".join(b"%d" % rp.mix(131 * k + j + 1) for j in range(64))
    elif kind == 1:
        x = bytes(c for c in lp.text(k, 4 * n) if 0x61 <= c <= 0x7A)
    elif kind == 2:
        x = b"w%05d " % k + lp.text(9000 + k, n)
    else:
        x = b"%05d" % k + b"xyzq#="[k // TRIP_KINDS % 6:][:1] * n
    assert len(x) >= n
    return x[:n]


def wide_trip_lines(w):
    """for long_plant.msl2() merged WITHOUT the part switches — one packed segment, every line found by both Missions —: w + 2 wide
    lines, so that the segment lists 2 w + 4 wide records.  With w the wavefronts of measure_wide_kernel's grid (W) each wavefront
    takes two strings and some take three: the zeroing in measure_wide_finish_lane, the fence behind it and the sums kept across trips
    run.  A narrow line behind every seventh wide one: the list is shorter than the segment.
    The list's order is whatever the atomics made it, so any string may follow any other on a wavefront.  A counter left behind
    shows whatever the order: the next string's histogram then holds 256 counts too many or more.  Each of them falls on a value the
    next string lacks — `distinct` is too large — or on one it has, whose c x LG(c) grows by at least 2 x LG(2) = 2^17 units where one
    step of the entropy field is 16 n < 2^13 of them: the field moves, or T goes below zero, wraps, and the field saturates at 65535,
    which no string of ASCII has.  uncleared() is that model; tests/test_measure_plant.py runs it over every pair of alphabets."""
    narrow = rp.lines((w + 2) // TRIP_NARROW + 1)
    out = []
    for k in range(w + 2):
        out.append(trip_line(k))
        if k % TRIP_NARROW == 3:
            out.append(narrow[k // TRIP_NARROW])
    return out


FOUR = ["\U0001F600", "\U00020000", "\U0001F4A9", "\U0002A6D6"]
SMALLEST_WIDE = (FOUR[0] * 64).encode()                           # 256 bytes in 64 characters: the one shape of a wide string at `-q 64`
LARGEST_NARROW = (FOUR[0] * 63 + "語").encode()                   # 255 bytes in 64 characters
LATE_TAIL, LATE_WIDE = 65, (0, 1, 63, 64)                         # the records behind the first r, and which of them are wide


def wide64(k):
    """64 four-byte characters, a function of k"""
    return "".join(FOUR[rp.mix(64 * k + j + 1) % 4] for j in range(64)).encode()


def steer(at, k):
    """a short ASCII line at `at` behind which two lines of 256 bytes in a row begin where long_plant.fitted() leaves them"""
    n = next(n for n in range(12, 24) if (at + n + 1) % 128 not in (124, 125, 126, 127, 0))
    return (b"steer %d " % k + b"=" * n)[:n]


def late_wide_lines(r):
    """for long_plant.msw() on the wave path (`-q 64`, every valid character passes, one packed segment), r + LATE_TAIL records: record
    0 is SMALLEST_WIDE and record 1 LARGEST_NARROW, its neighbour in bytes and in place; the others of the first r are fold_plant's
    lines, narrow.  Of the LATE_TAIL records behind them those at LATE_WIDE are wide.  With r the records of one trip of
    measure_narrow_kernel (R) the kernel's second trip has two wavefronts: the first lists its lanes 0, 1 and 63, the second its
    lane 0 — wave_reserve behind the one entry of trip 1, across a wavefront's end, with `w` beyond the first trip's wavefronts.
    long_plant.fitted() lays the lines; a steer() line keeps it from moving the wide ones of the tail from their places."""
    assert r >= 8
    body = lp.fitted([LARGEST_NARROW] + fp.lines(max(r, 400)), fp.Q, at=len(SMALLEST_WIDE) + 1)[:r - 2]
    out = [SMALLEST_WIDE] + body
    out.append(steer(sum(len(x) + 1 for x in out), 0))
    short = [x for x in fp.lines(400) if len(x) <= fp.Q][:LATE_TAIL - 5]
    out += [wide64(1), wide64(2)] + short
    out.append(steer(sum(len(x) + 1 for x in out), 1))
    out += [wide64(3), wide64(4)]
    assert len(out) == r + LATE_TAIL and lp.fitted(out[1:], fp.Q, at=len(SMALLEST_WIDE) + 1) == out[1:]
    assert [i for i, x in enumerate(out) if len(x) > NARROW_MAX] == [0] + [r + p for p in LATE_WIDE]
    return out


WORD_COUNTS = (33, 63, 64, 65, 127, 128, 129)
WORD_EDGE_LINES = 1600


def sized(head, seed, n):
    """n bytes: `head`, then text"""
    return (head + lp.text(seed, n))[:n]


def word_edge_lines():
    """for long_plant.msl2() merged, one segment, strings back to back in a 256-byte aligned arena: a string's place modulo 8 — the
    `head` of measure_load — is the sum of the lengths in front of it modulo 8.  The lengths are a function of the line's number that
    walks that sum through every residue beside every length that matters: 497 .. 520 bytes (63, 64 or 65 aligned words, by the
    head), 256 .. 264 (33), 1009 .. 1024 (127, 128, and 129: 1024 bytes at a head that is not 0), 4 .. 7 (inside one aligned word, or
    across two), 8 .. 255 (narrow, every pair of ends), 300 .. 899.  word_edges() says what a result's strings cover;
    tests/test_measure_plant.py asserts on the oracle's rows that nothing is missing, tests/test_gpu_measure_edges.py on the records
    in HBM."""
    out = []
    for i in range(WORD_EDGE_LINES):
        m, kind = rp.mix(i + 1), i % 8
        n = (497 + m % 24, 4 + m % 4, 8 + m % 248, 256 + m % 9, 497 + m % 24, 1009 + m % 16, 8 + m % 60, 1024 if i % 16 == 7 else 300 + m % 600)[kind]
        out.append(sized(b"%04d" % i, 5000 + i, n))
    return out


def word_edges(head, length):
    """what strings of these head alignments and lengths put in front of the lane functions: {(aligned words, head)} of the wide ones
    — words by the formula of measure_words —, {(head, bytes in the last word)} of the wide and of the narrow ones, and {(head,
    length)} of the narrow ones of 4 to 7 bytes that lie inside one aligned word"""
    counts, wide_ends, narrow_ends, inside = set(), set(), set(), set()
    for h, n in zip(head, length):
        words, last = (h + n + 7) >> 3, (h + n - 1) % 8 + 1
        if n > NARROW_MAX:
            counts.add((words, h))
            wide_ends.add((h, last))
        else:
            narrow_ends.add((h, last))
            if 4 <= n <= 7 and h + n <= 8:
                inside.add((h, n))
    return counts, wide_ends, narrow_ends, inside


def word_edges_complete(head, length):
    """assert that word_edges() holds everything word_edge_lines() is planted for"""
    counts, wide_ends, narrow_ends, inside = word_edges(head, length)
    every = {(h, t) for h in range(8) for t in range(1, 9)}
    assert {w for w, _ in counts} >= set(WORD_COUNTS), sorted({w for w, _ in counts})
    assert {(w, h) for w in (64, 65) for h in range(8)} <= counts and any(w == 129 and h for w, h in counts)
    assert wide_ends == every and narrow_ends == every, (sorted(every - wide_ends), sorted(every - narrow_ends))
    assert inside == {(h, n) for n in range(4, 8) for h in range(9 - n)}, sorted(inside)


RESET_WIDE, RESET_NARROW = 160, 40      # windows of 4096 bytes: 8 wide lines each, then 32 narrow lines each


def reset_lines():
    """for long_plant.msl2() under SX_MERGE_PART_FINDINGS=1024 (the parts are cut at windows of the input: merge_parts()): RESET_WIDE
    windows of 8 wide lines — 2560 records, more than two parts' worth —, then RESET_NARROW windows of 32 narrow lines, 2560 records
    again.  Every window's lines fill it exactly, and the cuts fall on multiples of 20 windows: eight segments of wide strings alone,
    then two without any — the first of them directly behind a segment of nothing else, with nothing but the cursor's reset between
    the list of the one and the empty list of the other."""
    out = []
    for s in range(RESET_WIDE):
        lens = [450 + rp.mix(8 * s + j + 1) % 91 for j in range(7)]
        lens.append(4096 - sum(lens))
        out += [sized(b"W%05d " % (8 * s + j), 100 * s + j, n - 1) for j, n in enumerate(lens)]
    for s in range(RESET_NARROW):
        for j in range(16):
            d = rp.mix(16 * s + j + 1) % 100
            out += [sized(b"n%05d " % (32 * s + 2 * j), 7 * s + j, 127 - d), sized(b"n%05d " % (32 * s + 2 * j + 1), 9 * s + j, 127 + d)]
    assert sum(len(x) + 1 for x in out) == 4096 * (RESET_WIDE + RESET_NARROW)
    return out


def merge_parts(position, nbytes, data_len, part_findings=1024, part_bytes=1 << 20):
    """per part of a merged result how many records it holds, as merge_plan cuts them (stringsext_amd/csrc/sx_merge.cpp): K parts by
    the switches' sizes, cut at the windows n_windows x j / K of the input — a record lies where its position puts it —, K doubled
    while a part holds more than twice the findings asked for.  position: the records' in merged order; nbytes: of all strings"""
    windows, total = -(-data_len // 4096), len(position)
    k = max(1, -(-nbytes // part_bytes), -(-total // part_findings))
    while True:
        k = min(k, windows)
        cuts = [windows * j // k * 4096 for j in range(1, k)]
        part = [bisect.bisect_right(cuts, int(p)) for p in position]
        assert part == sorted(part)                                      # (merged order goes window by window)
        sizes = [part.count(j) for j in range(k)]
        if max(sizes) <= 2 * part_findings or k >= windows:
            return sizes
        k *= 2
