"""The rule of sx_result_measure_device and sx_measure_bytes restated in Python as include/stringsext_amd.h states it — lg16() and
measure(), the oracle of every word in the tests (tests/test_measure_core.py on the CPU, tests/test_gpu_measure_device.py on the
device) —, and the planted lines that put strings at the edges of the two kernels: a LANE measures a string of at most 255 bytes with
one-byte counters, a WAVEFRONT a longer one.  Everything is a function of a line's place: no random state.  Expected findings come
from the oracle alone (result_plant.expected()); tests/test_measure_plant.py asserts on its strings what the lines are planted for."""
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
LEFTOVER = b"leftover? no: " + b"q" * 20                         # behind a wide line full of q: a counter that was not cleared would show


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
    EDGE_LENGTHS, SEVENS, PRINTABLE, and LEFTOVER behind a wide line full of its letter; WIDE_RUN wide lines in a row: wherever a part ends among
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
