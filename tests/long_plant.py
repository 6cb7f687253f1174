"""A planted buffer of LONG lines whose findings are known line by line, for the kernels that work on a result lying in HBM
(tests/test_long_plant.py on the CPU, tests/test_gpu_result_long_strings.py on the device): what tests/result_plant.py is for many short
strings, this is for strings of up to 1024 bytes — and, in the source `limit`, of 16 000 and 64 000 bytes.  Everything is a function of
a line's place: no random state.  Expected findings come from the oracle alone (result_plant.expected()).

The sources
 msl2()   two Missions, `-e ascii -e utf-8 -n 4 -q 1024`, over lines(): ASCII only, so every line is found once by each Mission
          (merged, packed records)
 msl1()   one Mission, `-e utf-8 -n 4 -q 255` (the longest line the device's lane-per-region replay takes), over one_lines(): the
          lines() of at most 255 bytes and utf8_lines(), 255 characters in up to 1000 bytes
 msw()    one Mission, `-e utf-8 -n 4 -q 64` with a filter that lets every valid character pass, over wave_lines(): at most 64
          characters and up to 256 bytes a line
 limit_ms()   two Missions at `-q 16000` over limit_lines()

What lines() holds (tests/test_long_plant.py asserts each on the oracle's strings)
 lengths    every byte length of LENGTHS, and every length modulo 16
 families   groups of lines that share a stem of S bytes and part at byte S, S in STEMS; in each a line that is a proper prefix of the
            others at a multiple of 8 bytes, exact copies (classes of 1, 2 and 3 or more), and upper-case copies, equal only under the
            fold.  The family of STEM_LONG also holds two lines of 1024 bytes that differ in their last byte alone.
 tiers      filler lines whose lengths are chosen so that the number of undecided groups (groups_left()) passes 257, 17, 5, 3 and 2
 tokens     NEEDLE at offset 0, as the last bytes of a line of 1024, and at every offset 1000 .. 1015 of sixteen lines of 1024 (one of
            them straddles a 16-byte boundary wherever the strings lie); the same for NEEDLE64, of the longest length a substring
            selection takes, and KEYWORD255.  Every token is also SPLIT: its first half ends one line and its second half begins the
            next, and the strings lie back to back — a match must not span two findings.
 density    DENSE: 100 matches of EXTRACTS[0] in one line; ONE_MATCH: one match of 1003 bytes; RUN: 600 times the digit 7, in which
            `77` stands at 599 overlapping places and `777` at 598
utf8_lines() adds lines with bytes >= 0x80 at the first and at the last byte of an 8-byte word, a family whose stem is Cyrillic, and a
family whose stem is 240 four-byte characters, with NEEDLE behind byte 900."""
import result_plant as rp
import refconfig as rc

NEEDLE = b"{needle}"
NEEDLE64 = b"<" + b"0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"[:62] + b">"       # 64 bytes: the longest substring pattern
KEYWORD255 = b"[" + bytes(0x21 + (i * 7 + i // 13) % 90 for i in range(253)).replace(b"[", b"!").replace(b"]", b"!") + b"]"
TOKENS = [NEEDLE, NEEDLE64, KEYWORD255]
LENGTHS = (7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024)
STEMS = (23, 24, 25, 255, 256, 257, 1000)
STEM_LONG = 1000
GROUP_COUNTS = (2, 3, 5, 17, 257)                      # 2^k + 1: where a group key one bit too narrow merges two groups
EXTRACTS = [rb"[0-9]{5,}", rb"uid="]                  # (result_plant's)
REGEXES = [rb"^fam[0-9]+ ", rb"tail[0-9]$", rb"^stem1000 [a-z0-9 .:=/]*[A-Z]", rb"uid=10:[0-9]+ "]
LABELS = [rb"^fam", rb"[0-9]$", rb"\{needle\}", rb"[0-9]{5}", rb"^.{200,}$", rb"uid=10"]
TALLY = [b"77", b"777", b"7" * 255, NEEDLE, KEYWORD255, b"uid=", b"fam", b":", b"no such keyword", b"tail"]
WORDS = [b"open", b"read", b"stat", b"exec", b"mmap", b"conn", b"uid=10", b"key=7", b"/tmp/x", b"/var/log", b"pid=311", b"mode=0644", b"eth0", b"net:"]


def msl2():
    return rc.missions(encodings=["ascii", "utf-8"], chars_min="4", output_line_len="1024")


def msl1():
    # (-q 255 is the longest line the lane-per-region replay takes on the device, stringsext_amd/csrc/sx_stage_b.cpp: a Mission with a
    # longer one is replayed on the host, and its result never lies in HBM as sx_finding records)
    return rc.missions(encodings=["utf-8"], chars_min="4", output_line_len="255", unicode_block_filter="0x%x" % rc.UBF_ALL_VALID)


def msw():
    # (the alias "All" would resolve to All-Asian: the first prefix match wins)
    return rc.missions(encodings=["utf-8"], chars_min="4", output_line_len="64", unicode_block_filter="0x%x" % rc.UBF_ALL_VALID)


def limit_ms():
    return rc.missions(encodings=["ascii", "utf-8,,,0x%x" % rc.UBF_ALL_VALID], chars_min="4", output_line_len="16000")


def text(seed, n):
    """n bytes of lower-case words, digits and punctuation, a function of `seed`; no upper-case letter, no `{`, `<`, `[` and no run of
    five digits"""
    out, k, have = [], seed, 0
    while have < n:
        k = rp.mix(k + 1)
        w = WORDS[k % len(WORDS)] + (b":%x" % (k // 64 % 4096) if k % 3 else b"") + b" "
        out.append(w)
        have += len(w)
    return b"".join(out)[:n]


def family(s, name):
    """the lines of the family whose stem has s bytes: they share [0, s) and differ at byte s"""
    head = b"%s " % name
    stem = head + text(s, s - len(head))
    assert len(stem) == s
    cut = (s + 8) // 8 * 8                                       # the first multiple of 8 behind the parting byte
    a, b, c = stem + b"a" + text(s + 1, cut - s - 1), stem + b"b" + text(s + 2, cut - s - 1), stem + b"c" + text(s + 3, 30)
    return [a + b" tail1", b + b" tail2", c, a, a + b" tail1", b + b" tail2", a + b" tail1", a + b" tail3", (a + b" tail1").upper(), c.upper(), stem]


def long_family():
    """the family of STEM_LONG: every line of 1008 bytes or more shares its first 1000 bytes"""
    s = STEM_LONG
    head = b"stem1000 "
    stem = head + text(s, s - len(head))
    a, b = stem + b"a" + text(1, 23), stem + b"b" + text(2, 23)
    out = [a, b, a[:1023] + b"#", a[:1016] + text(3, 8), a[:1016], a[:1023], a, b, a, a[:1000] + a[1000:].upper(), stem, stem + b"a" + text(1, 7)]
    out += [stem + b"c" + text(4, 24 - 1 - len(tok)) + tok if len(tok) <= 23 else stem[:1024 - len(tok)] + tok for tok in TOKENS]      # the last bytes of a line of 1024
    for tok in TOKENS:
        n = len(tok)
        if n <= 16:
            out += [stem + text(5 + j, j) + tok + text(6, 24 - j - n) for j in range(16)]        # at the offsets 1000 .. 1015
        else:                                                                                     # (longer than 16 bytes: it straddles a boundary wherever it lies)
            out.append(stem[:1010 - n] + tok + text(6, 14))                                       # it ends at offset 1010
    assert all(len(x) in (1000, 1008, 1016, 1023, 1024) for x in out), [len(x) for x in out]
    return out


DENSE = b" ".join(b"%05d" % (10007 * i % 100000) for i in range(100))                # 100 matches of [0-9]{5,}: more than a wavefront has lanes
ONE_MATCH = b"9" * 1003                                                               # one match, 1003 bytes
RUN = b"run " + b"7" * 600 + b" end"


def token_lines(tok, k):
    """the token at offset 0, and split between two neighbours: neither line holds it"""
    h = len(tok) // 2
    return [tok + b" first " + text(k, 40), text(k + 1, 30 + k % 7) + b" " + tok[:h], tok[h:] + b" " + text(k + 2, 25), text(k + 3, 20)]


def tier(base, count, lo, hi):
    """`count` different lines of lo .. hi - 1 bytes: `tier` and a number, then text"""
    out = []
    for i in range(count):
        head = b"t%d:%04d " % (base, i)
        out.append(head + text(base * 1000 + i, lo + rp.mix(base * 1000 + i) % (hi - lo) - len(head)))
    return out


# how many filler lines each tier has: chosen so that groups_left() passes GROUP_COUNTS (tests/test_long_plant.py asserts it)
TIERS = ((1, 900, 4, 200), (2, 227, 272, 500), (3, 10, 520, 600), (4, 2, 640, 648), (5, 1, 664, 672))

_lines = []
HEAD = 30 + 3 * 11 + 15 + 15 + 30      # the lines of head(): filler, three families, the dense lines and the tokens, the long family's first lines, filler


def lines():
    """every ASCII line, in buffer order: a head that holds something of every kind (the harness tests and the small GPU sources take
    prefix(HEAD)), then the filler with the other families, the long lines and the ladder of lengths spread over it, then copies of
    lines of the head — members of one class lie far apart, in different parts of a merged result"""
    if _lines:
        return list(_lines)
    fams = [family(s, b"fam%04d" % s) for s in STEMS[:-1]]
    longs = long_family()
    special = [DENSE, ONE_MATCH, RUN]
    for k, tok in enumerate(TOKENS):
        special += token_lines(tok, 100 + 10 * k)
    ladder = [b"%04d:" % n + text(n, n - 5) for n in LENGTHS if n < 1000]
    fill = [x for t in TIERS for x in tier(*t)]
    out = fill[:30] + fams[0] + fams[1] + fams[2] + special + longs[:15] + fill[30:60]
    assert len(out) == HEAD
    spread = [x for f in fams[3:] for x in f] + longs[15:] + ladder
    fill = fill[60:]
    step, at = max(1, len(fill) // (len(spread) + 1)), 0
    for i, x in enumerate(fill):
        out.append(x)
        if i % step == step - 1 and at < len(spread):
            out.append(spread[at])
            at += 1
    out += spread[at:] + [longs[0], longs[1], fams[0][0], fams[3][0], fams[3][2], longs[0]]
    _lines.extend(out)
    return list(out)


def fitted(ls, q, at=0):
    """the reference decodes a window of 4096 bytes in slices of 2 q bytes, and a line of multi-byte characters that begins in the last three bytes of a slice
    or at its first is cut behind its first slice: a short filler line moves such a line on.  at: where in the buffer the lines begin"""
    out = []
    for k, x in enumerate(ls):
        if len(x) > q and at % 4096 % (2 * q) in (2 * q - 3, 2 * q - 2, 2 * q - 1, 0):
            out.append(b"fill %d" % (k % 10))
            at += 7
        out.append(x)
        at += len(x) + 1
    return out


def utf8_lines():
    """lines for the one-Mission source: bytes >= 0x80 at an 8-byte word's first and last byte, a Cyrillic family, upper case that no
    ASCII fold touches, and a family of 255 characters in 1000 bytes and more: a stem of 240 four-byte characters, copies, lines that
    differ in their last byte, NEEDLE as the last bytes and at sixteen neighbouring offsets behind byte 900"""
    e = "é".encode()                                            # two bytes, both >= 0x80
    out = [b"1234567" + e + b"9abcdef" + e + b" first and last byte of a word",      # 0xC3 at byte 7 (a word's last), 0xA9 at byte 8 (a word's first)
           b"1234567" + e + b"9abcdef" + e + b" first and last byte of a worD",
           e + b"234567" + e + b" at byte 0 and at bytes 7, 8",
           b"12345678" + e + b"bcde" + e]                       # 0xA9 is the last byte of the line and of a word (16 bytes)
    stem = ("привет мир строка поиск " * 9).encode()
    out += [stem + "а".encode() + b" tail1", stem + "б".encode() + b" tail2", stem + "а".encode() + b" tail1", stem, stem + "А".encode() + b" tail1"]
    wide = b"wide4 " + "\U00020000".encode() * 240                # 966 bytes, 246 characters
    a, b = wide + b"a tail001", wide + b"b tail002"
    out += [a, b, a[:-1] + b"2", a, wide + b"A TAIL001", wide, a, b, wide + b"a" + NEEDLE, wide[:-4] + NEEDLE[:4], NEEDLE[4:] + wide[6:]]
    out += [wide[:-4 * 14] + text(20 + j, j) + NEEDLE + text(40, 15 - j) for j in range(16)]      # NEEDLE at the offsets 910 .. 925
    out += [b"run " + b"7" * 240 + b" end"]
    assert all(len(x.decode()) <= 255 for x in out)
    return out


def one_lines():
    """the lines of the one-Mission source: every line of lines() that has at most 255 characters, then utf8_lines()"""
    return fitted([x for x in lines() if len(x) <= 255] + utf8_lines(), 255)


def wave_lines():
    """lines of at most 64 characters and up to 256 bytes, of one-, two-, three- and four-byte characters"""
    three, four = ["語", "漢", "字", "文", "日", "本"], ["\U0001F600", "\U00020000", "\U0001F4A9", "\U0002A6D6"]
    out = []
    for i in range(260):
        k = rp.mix(i + 1)
        n = (64, 63, 48, 17, 5, 64, 33, 64)[i % 8]
        if i % 5 == 0:
            s = "".join(four[(k >> j) % 4] for j in range(n))                                    # 4 n bytes: up to 256
        elif i % 5 == 1:
            s = "".join(three[(k >> j) % 6] for j in range(n))
        elif i % 5 == 2:
            s = "".join((four[0] * 60 + three[(k >> j) % 6] + "abc")[j] for j in range(n))      # a stem of 60 four-byte characters: 240 bytes
        elif i % 5 == 3:
            s = ("wave %d " % (k % 50) + "".join((three + four + ["é", "я", "x", "7"])[(k >> j % 20) % 14] for j in range(n)))[:n]
        else:
            s = out[k % len(out)].decode() if i % 10 == 4 else ("uid=10 77777 " + four[k % 4] * 40)[:n]      # copies; tokens
        out.append(s.encode())
    out += [four[0].encode() * 63 + b"A", four[0].encode() * 63 + b"B", four[0].encode() * 64, four[0].encode() * 64, four[0].encode() * 60 + b"(nee"]
    h = len(NEEDLE) // 2
    out += [NEEDLE + three[0].encode() * 50, three[1].encode() * 60 + NEEDLE[:h], NEEDLE[h:] + four[1].encode() * 60, four[2].encode() * 56 + NEEDLE]
    assert all(len(x.decode()) <= 64 and len(x) <= 256 for x in out)
    return fitted(out, 64)


LIMIT_NEEDLE = "\U0001F600\U0001F4A9".encode()          # two four-byte characters


def limit_lines():
    """a handful of lines, among them one of 16 000 ASCII characters and one of 16 000 four-byte characters (64 000 bytes: the largest
    str_len of a packed record at that bound) whose last bytes are LIMIT_NEEDLE, its copy, and a line that differs from it in its last
    eight bytes alone"""
    stem = ("\U00020000" * 15998).encode()
    big, other = stem + LIMIT_NEEDLE, stem + LIMIT_NEEDLE[4:] + LIMIT_NEEDLE[:4]
    return [b"limit first line", text(9, 16000), b"between the two", big, text(9, 16000), b"limit last line", text(9, 15999) + b"#", other, big]


def buffer(ls):
    return b"\n".join(ls) + b"\n"


def prefix(n):
    """the buffer of the first n lines()"""
    return buffer(lines()[:n])


def groups_left(strs, fold=None, descending=False):
    """a plain model of the order's refinement, after the rule at the top of stringsext_amd/csrc/sx_order_core.hpp: round d gives every
    undecided item the word (w, rem) of the bytes [8d, 8d + 8) of its (folded) string — descending: (~w, 8 - rem) —, and the items of a
    group with equal words are a new group; a group of one is decided, and a group whose strings ended inside the word (rem < 8) is.
    So after round d an item is undecided iff its string has at least 8 (d + 1) bytes and another item shares them.  Returns the
    number of undecided groups after round 0, 1, ... until none is left."""
    keys = [fold(s) if fold else s for s in strs]
    groups, out, d = [list(range(len(keys)))], [], 0
    while True:
        split = []
        for g in groups:
            new = {}
            for i in g:
                part = keys[i][8 * d:8 * d + 8]
                w, rem = int.from_bytes(part.ljust(8, b"\x00"), "big"), len(part)
                new.setdefault((w ^ (1 << 64) - 1, 8 - rem) if descending else (w, rem), []).append(i)
            split += [m for m in new.values() if len(m) > 1 and len(keys[m[0]]) >= 8 * d + 8]
        if not split:
            return out
        out.append(len(split))
        groups, d = split, d + 1
