"""A planted buffer of UTF-8 lines in many scripts whose findings are known line by line, for the Unicode case fold of a result lying in
HBM (tests/test_fold_plant.py on the CPU, tests/test_gpu_fold_device.py on the device): what tests/result_plant.py is for ASCII lines.
Every line has 4 to 60 characters, at least chars_min and no more than an output line holds, so that a line is never cut; everything
is a function of the line number: no random state.  Expected findings come from the oracle alone (result_plant.expected()).

The sources
 ms1()   one Mission, `-e utf-8 -n 4 -q 64` with a filter that lets every valid character pass: line k is finding k
 ms2()   two Missions, `-e ascii -e utf-8 -n 4`: merged, packed records, several segments under SX_MERGE_PART_FINDINGS
 ms2v()  the same with the filter of ms1() on the UTF-8 Mission, for split_lines(); msl() the same at `-q 1024`, for long_lines(1024)

What the lines hold (tests/test_fold_plant.py asserts each)
 scripts    words in ASCII upper case, Latin-1, Greek with a final sigma, Cyrillic, Cherokee — whose folding is the UPPER case — and
            Deseret (four bytes a character)
 lengths    U+023A and U+023E, which GROW from two bytes to three; U+212A KELVIN SIGN and U+1E9E, which shrink
 unchanged  'ß' and 'İ', which have only a full folding, and CJK
 the fold   one line of five is the upper case of an earlier line, character by character where that is one character: the fold joins
            classes that the byte comparison and the ASCII fold keep apart
 words      EDGES: a two-byte character behind 0 .. 8 ASCII bytes and sixteen more in front of the next, so that wherever a string
            lies a byte >= 0x80 stands at the first and at the last byte of an 8-byte word; eight ASCII bytes and more between them
 needles    NEEDLES, in upper, lower and mixed case: what `grep -i` looks for

Behind them, for tests/test_gpu_fold_edges.py, what the lines above do not reach on the device
 page_lines()    every code point of every page of the fold's table and its neighbours on no page, and code points above the table
 split_lines()   characters that SPLIT_PATTERNS cut in two: an extraction's matches lie back to back, a lead byte in front of the
                 next match's continuation bytes
 long_lines(q), limit_lines()   lines of q characters and of 16 000 that grow, shrink and keep their length

fold() is the rule of sx_fold_utf8 written in Python as include/stringsext_amd.h states it: the oracle of every fold in the tests."""
import re

import numpy as np

import long_plant as lp
import refconfig as rc
import result_plant as rp

Q = 64


def ms1():
    # (the alias "All" would resolve to All-Asian: tests/long_plant.py)
    return rc.missions(encodings=["utf-8"], chars_min="4", output_line_len=str(Q), unicode_block_filter="0x%x" % rc.UBF_ALL_VALID)


def ms2():
    return rc.missions(encodings=["ascii", "utf-8"], chars_min="4")


def ms2v():
    """ms2() with a UTF-8 Mission that lets every valid character pass (the default filter ends a finding in front of U+212A and
    U+10400): the Missions of split_lines()"""
    return rc.missions(encodings=["ascii", "utf-8,,,0x%x" % rc.UBF_ALL_VALID], chars_min="4")


def fold_char(x):
    """Unicode simple case folding of one character, from unicodedata: CaseFolding.txt's statuses C and S"""
    if 0xD800 <= ord(x) <= 0xDFFF:
        return x                      # (an escaped byte)
    f = x.casefold()
    if len(f) == 1:
        return f
    f = x.lower()
    return f if len(f) == 1 else x


_fold_table = {}


def fold(b):
    """SX_FOLD_SIMPLE of a byte string"""
    if not _fold_table:
        _fold_table.update({c: fold_char(chr(c)) for c in range(0x110000) if fold_char(chr(c)) != chr(c)})
    return b.decode("utf-8", "surrogateescape").translate(_fold_table).encode("utf-8", "surrogateescape")


def upper(s):
    """the upper case of a str, character by character, where that is one character"""
    return "".join(c.upper() if len(c.upper()) == 1 else c for c in s)


NEEDLES = ["ПАРОЛЬ", "ÅNGSTRÖM", "ΑΘΉΝΑ", "PASSWORD"]
WORDS = ["PASSWORD", "Password", "Login", "ADMIN", "root", "Key=7", "TMP/X",                      # ASCII
         "ÅNGSTRÖM", "ångström", "École", "ÑANDÚ", "Straße", "STRASSE",               # Latin-1; ß has only a full folding
         "ΑΘΉΝΑ", "Αθήνα", "ΟΔΥΣΣΕΎΣ", "οδυσσεύς", "ΣΊΣΥΦΟΣ",                          # Greek: the final sigma folds to σ
         "ПАРОЛЬ", "пароль", "Привет", "МИР", "Ёж",                                   # Cyrillic
         "ᏣᎳᎩ", "ꮃꭳꭹ", "ᎠᏂᏴᏫᏯ",                                         # Cherokee: the small letters fold to the capitals
         "\U00010400\U00010401\U00010402", "\U00010428\U00010429\U0001042a", "\U00010414\U0001043c",      # Deseret
         "ȺȾ", "aȺb", "ⱥⱦ",                                  # U+023A, U+023E grow 2 -> 3 bytes
         "Kelvin", "\u212Aelvin", "\u1E9E", "GRO\u1E9E",                           # U+212A KELVIN SIGN 3 -> 1 byte, U+1E9E 3 -> 2
         "\u0130stanbul", "ISTANBUL", "漢字", "日本語", "\u00B5m", "\u03A9", "\u2126"]      # İ stays; CJK; micro and ohm fold to Greek letters
EDGES = ["x" * j + "Ж" + "ABCDEFGHIJKLMNOP" + "Й" + "QRSTUVWXYZ012345" + "é" for j in range(9)]

_lines = []
_at = [0]


def raw(k):
    """what line k would be if it were no copy"""
    if k % 37 == 5:
        return EDGES[k // 37 % len(EDGES)]
    m, out, n = rp.mix(k + 1), [], 0
    want = 4 + m % 57                                                  # characters: 4 .. 60
    while True:
        m = rp.mix(m + 1)
        w = WORDS[m % len(WORDS)] + (":%x" % (m // 64 % 4096) if m % 4 == 0 else "")
        if n + len(w) + (1 if out else 0) > want:
            break
        out.append(w)
        n += len(w) + (1 if len(out) > 1 else 0)
    s = " ".join(out)
    return s + "#" * max(0, 4 - len(s)) if len(s) < 4 else s


def lines(n):
    """the first n lines, as bytes.  (The reference decodes a window of 4096 bytes in slices of 2 q bytes, and a line of multi-byte
    characters longer than q bytes that begins in the last three bytes of a slice or at its first is cut behind its first slice:
    a short line of its own stands in front of such a line — tests/long_plant.py fitted().)"""
    out = _lines
    while len(out) < n:
        k = len(out)
        if k % 5 == 3 and k > 3:
            s = upper(out[rp.mix(k) % k].decode())
        elif k % 11 == 7:
            s = out[k - 1 - rp.mix(k) % min(k, 500)].decode()              # a copy: classes of two and more
        else:
            s = raw(k)
        x = s.encode()
        if len(x) > Q and _at[0] % 4096 % (2 * Q) in (2 * Q - 3, 2 * Q - 2, 2 * Q - 1, 0):
            x = b"fill %d" % (k % 10)
        assert 4 <= len(x.decode()) <= 60
        out.append(x)
        _at[0] += len(x) + 1
    return out[:n]


def buffer(n):
    """n lines"""
    return b"\n".join(lines(n)) + b"\n"


# ---- what only the device has: the whole table in LDS, strings that lie back to back, long strings (tests/test_gpu_fold_edges.py)

def pages():
    """the numbers c >> 7 of the table's pages, as stringsext_amd/csrc/gen_fold_table.py derives them: where some code point folds"""
    fold(b"")
    return sorted({c >> 7 for c in _fold_table})


EXTRA_POINTS = [0x1E97F, 0x1E980, 0x1E981, 0x1F600, 0x20000, 0x10FFFF, 0xD7FF, 0xE000, 0xFFFD]      # around kFoldLimit, far above it, around the surrogates


def page_points():
    """every code point >= 0x80 of every page, in front of and behind each page its neighbour where that lies on no page (the index says
    kFoldNoPage there) and is a scalar value, then EXTRA_POINTS: 4394 entries, two of EXTRA_POINTS for the second time"""
    on, out = set(pages()), []
    for p in pages():
        below, above = (p << 7) - 1, (p + 1) << 7
        out += [below] if below >= 0x80 and below >> 7 not in on else []
        out += [c for c in range(p << 7, above) if c >= 0x80]
        out += [above] if above >> 7 not in on else []
    assert not any(0xD800 <= c <= 0xDFFF for c in out)
    return out + EXTRA_POINTS


def page_lines():
    """page_points(), 48 to a line behind a tag, for ms1(): whatever the table holds, and what it does not hold next to it"""
    pts = page_points()
    return lp.fitted([b"pg%02d " % (i // 48) + "".join(map(chr, pts[i:i + 48])).encode() for i in range(0, len(pts), 48)], Q)


# Lines whose extraction cuts characters in two.  An item is an upper-case word, a digit that says where the cut goes, the character,
# an upper-case word; SPLIT_PATTERNS take the item apart behind the first k bytes of the character, so that the left half ends one
# match and the right half begins the very next one — and the matches of a result lie back to back in the arena.
SPLIT_CHARS = {1: "Ж\u023A", 2: "\u212A", 3: "\u212A", 4: "\U00010400", 5: "\U00010400", 6: "\U00010400"}      # digit: the characters it stands in front of
SPLIT_CUTS = {1: (2, 1), 2: (3, 1), 3: (3, 2), 4: (4, 1), 5: (4, 2), 6: (4, 3)}                  # digit: (the sequence's bytes, those left of the cut)
SPLIT_PATTERNS = [rb"[A-Z]+1[\xc8\xd0]", rb"[A-Z]+2\xe2", rb"[A-Z]+3\xe2\x84", rb"[A-Z]+4\xf0", rb"[A-Z]+5\xf0\x90", rb"[A-Z]+6\xf0\x90\x90",
                  rb"[A-Z]+8\xd0",                  # the last line: its match ends in a lead byte, and nothing takes the byte behind it
                  rb"[\x80-\xbf]+[A-Z]+",           # the right halves
                  rb"\xc8", rb"\xba"]               # U+023A behind any other digit: a lone lead byte, then a lone continuation byte
SPLIT_LAST = "EN8Ж"                                 # (three ASCII characters: the ASCII Mission of ms2() finds nothing in it)
SPLIT_WORDS = ["ABC", "PASSWD", "KEY", "ADMIN", "QRSTUV", "TMP", "LOGIN"]


def split_lines(n=60):
    """n lines of two or three items each, every digit and every character of SPLIT_CHARS in turn, some with `7` and U+023A: the two lone
    bytes; then SPLIT_LAST.  At most 60 bytes a line.  (A cut leaves a lead byte with too few continuation bytes and continuation bytes
    without a lead byte.  The narrowed second bytes of E0, ED, F0 and F4, and overlong forms, cannot arise by cutting valid text: they
    stay pinned on the host only, tests/test_fold_core.py.)"""
    out = []
    for k in range(n):
        m, items = rp.mix(k + 1), []
        for j in range(2 + k % 2):
            d = 1 + (2 * k + j) % 6
            ch = SPLIT_CHARS[d][(k // 3 + j) % len(SPLIT_CHARS[d])]
            items.append("%s%d%s%s" % (SPLIT_WORDS[(m >> j) % 7], d, ch, SPLIT_WORDS[(m >> j + 3) % 7]))
        if k % 4 == 1:
            items.append("X7\u023A")
        x = " ".join(items).encode()
        assert len(x) <= 60, x
        out.append(x)
    return out + [SPLIT_LAST.encode()]


SPLIT_BEHIND = 3000      # the lines() in front of split_lines() in the merged source: several segments


def split_buffer():
    return buffer(SPLIT_BEHIND) + lp.buffer(split_lines())


def split_rx():
    """SPLIT_PATTERNS as one pattern of Python's re: its matches are grep -oE's.  (Leftmost-longest is Python's leftmost-first here: at
    a letter one pattern at most matches, by the digit behind the word, and at a continuation byte the pattern of the right halves
    stands in front of the lone byte's.)"""
    return re.compile(b"|".join(b"(?:" + p + b")" for p in SPLIT_PATTERNS))


def split_pairs(strs):
    """(every match of SPLIT_PATTERNS in strs, in order; per cut (n, k) how many matches end in the first k bytes of a sequence of n
    whose other bytes begin the very next match of the same string — the next string of the extraction's arena)"""
    rx, found, cuts = split_rx(), [], {}
    for s in strs:
        prev = None
        for m in rx.finditer(s):
            if prev is not None and prev.end() == m.start() and cut_of(prev.group(), m.group()):
                cuts[cut_of(prev.group(), m.group())] = cuts.get(cut_of(prev.group(), m.group()), 0) + 1
            prev = m
            found.append(m.group())
    return found, cuts


def cut_of(a, b):
    """(n, k) where match `a` ends in the first k bytes of a sequence of n and its neighbour `b` begins with the other n - k; or None"""
    k = next((k for k in (1, 2, 3) if len(a) >= k and a[-k] >= 0xC2), None)
    if k is None or any(x & 0xC0 != 0x80 for x in a[len(a) - k + 1:]):
        return None
    n = 2 if a[-k] < 0xE0 else 3 if a[-k] < 0xF0 else 4
    if k < n and len(b) >= n - k and all(x & 0xC0 == 0x80 for x in b[:n - k]) and fold(a) + fold(b) != fold(a + b):
        return n, k
    return None


LONG_CHARS = ["\u023A", "\u212A", "\U00010400"]      # two bytes that grow to three, three that shrink to one, four whose last changes


def msl():
    """two Missions at `-q 1024`, the UTF-8 one with a filter that lets every valid character pass: merged, packed records"""
    return rc.missions(encodings=["ascii", "utf-8,,,0x%x" % rc.UBF_ALL_VALID], chars_min="4", output_line_len="1024")


def long_lines(q):
    """for `-q q`: q times each of LONG_CHARS; for j = 0 .. 8 j times U+023A, ABCDEFGH as often as q lets a line be (120 times at
    most), U+212A — behind j grown characters the output is j bytes further on than the input —; and eight lines of U+023A and 16
    ASCII bytes, which hold an aligned 8-byte word wherever they lie.  A result's strings lie back to back, and so do their folds:
    each of the eight lies one byte further on against its source than the one before, so the words of ASCII go out by every store
    of FoldWrite::word whatever the first one's place.  (At q = 255 the lines of j characters alone leave out the places that are
    four bytes off.)"""
    reps = min(120, (q - 9) // 8)
    out = [b"long %d first line" % q] + [(c * q).encode() for c in LONG_CHARS]
    out += [("\u023A" * j + "ABCDEFGH" * reps + "\u212A").encode() for j in range(9)]
    out += [("\u023Aword %d ABCDEFGHI" % j).encode() for j in range(8)]
    return lp.fitted(out + [b"long last line"], q)


LIMIT_Q = 16000


def limit_lines():
    """for long_plant.limit_ms(), `-q 16000`: a line that grows from 32 000 bytes to 48 000 (a packed str_len behind 2^15), one that shrinks
    from 48 000 to 16 000, one of 64 000 bytes of which the fold changes every fourth, 16 000 bytes of ASCII, and one character that
    grows in the middle of 15 999 ASCII bytes: every word behind it goes out one byte further on.  (The long lines move what follows
    them by multiples of eight bytes; the three characters that grow in a short line move the words of ASCII behind them by three,
    and the one character by four.)"""
    q = LIMIT_Q
    out = [b"limit first line", ("\u023A" * q).encode(), b"grown", ("\u212A" * q).encode(), b"shrunk", ("\U00010400" * q).encode(), b"four bytes",
           b"ABCDEFGH" * (q // 8), "\u023A\u023A\u023A three grow".encode(), b"A" * (q // 2 - 1) + "\u023A".encode() + b"B" * (q // 2), b"limit last line"]
    return lp.fitted(out, q)


def word_places(x, p_in, p_out):
    """of the string x at the address p_in, whose fold goes to p_out: the addresses to which its 8-byte words go that are 8-byte
    aligned, lie wholly in x and hold ASCII only — what fold_walk folds as a word, and FoldWrite::word stores by the place's alignment"""
    nb = []
    for y in (x, fold(x)):
        c = np.fromiter(map(ord, y.decode("utf-8", "surrogateescape")), dtype=np.int64)
        nb.append(np.where(c < 0x80, 1, np.where(c < 0x800, 2, np.where((c >= 0xDC80) & (c <= 0xDCFF), 1, np.where(c < 0x10000, 3, 4)))))
    assert len(nb[0]) == len(nb[1]) and int(nb[0].sum()) == len(x)
    start_in, start_out = np.cumsum(nb[0]) - nb[0], np.cumsum(nb[1]) - nb[1]
    high = np.concatenate([[0], np.cumsum(np.frombuffer(x, dtype=np.uint8) >= 0x80)])
    k = np.arange(-p_in % 8, len(x) - 7, 8, dtype=np.int64)
    k = k[high[k + 8] == high[k]]                                      # ASCII only: byte k begins a character
    return p_out + start_out[np.searchsorted(start_in, k)]


def word_stores(strs, src, dst):
    """how many such words of the strings `strs` at the addresses `src`, folded to `dst`, go to a place that is (8-byte aligned, 4-byte
    but not 8-byte aligned, neither)"""
    to = np.concatenate([word_places(x, int(a), int(b)) for x, a, b in zip(strs, src, dst)])
    return int((to % 8 == 0).sum()), int((to % 8 == 4).sum()), int((to % 4 != 0).sum())


def back_to_back(strs):
    """the offsets of strings that lie back to back"""
    n = np.array([len(x) for x in strs], dtype=np.int64)
    return np.cumsum(n) - n
