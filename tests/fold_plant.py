"""A planted buffer of UTF-8 lines in many scripts whose findings are known line by line, for the Unicode case fold of a result lying in
HBM (tests/test_fold_plant.py on the CPU, tests/test_gpu_fold_device.py on the device): what tests/result_plant.py is for ASCII lines.
Every line has 4 to 60 characters, at least chars_min and no more than an output line holds, so that a line is never cut; everything
is a function of the line number: no random state.  Expected findings come from the oracle alone (result_plant.expected()).

The sources
 ms1()   one Mission, `-e utf-8 -n 4 -q 64` with a filter that lets every valid character pass: line k is finding k
 ms2()   two Missions, `-e ascii -e utf-8 -n 4`: merged, packed records, several segments under SX_MERGE_PART_FINDINGS

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

fold() is the rule of sx_fold_utf8 written in Python as include/stringsext_amd.h states it: the oracle of every fold in the tests."""
import refconfig as rc
import result_plant as rp

Q = 64


def ms1():
    # (the alias "All" would resolve to All-Asian: tests/long_plant.py)
    return rc.missions(encodings=["utf-8"], chars_min="4", output_line_len=str(Q), unicode_block_filter="0x%x" % rc.UBF_ALL_VALID)


def ms2():
    return rc.missions(encodings=["ascii", "utf-8"], chars_min="4")


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
