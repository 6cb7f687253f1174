"""The approximate match (sx_result_fuzzy_device, sx_fuzzy_bytes) restated in Python, and the planted cases of its tests
(tests/test_fuzzy_plant.py asserts what they hold, tests/test_fuzzy_core.py and tests/test_gpu_fuzzy_device.py use them).

The rule, as include/stringsext_amd.h states it: bit p of a string's word is set iff some substring of it has Levenshtein distance at
most k_p from pattern p — Sellers' table: row 0 all zeros, D[i][j] = min(D[i-1][j-1] + (P[i] != T[j]), D[i-1][j] + 1, D[i][j-1] + 1),
and the bit is set iff min_j D[m][j] <= k.  last_row() is that table and nothing else, computed ROW BY ROW: row i of ALL the texts of a
call at once, one numpy array over their bytes — column 0 of every text, D[i][0] = i, is an entry of its own in front of the text's
bytes.  The third term runs along the row: D[i][j] = min over j' <= j of (a[j'] + j - j'), a = the first two terms; that is a running
minimum of a[j'] - j', kept from crossing into the next text by an offset per text that makes every later text's entries smaller.
No bit vector, no automaton: nothing of the code under test.  words() memoises per set and distinct string.

Everything planted is a function of its arguments: no random state."""
import numpy as np

BIG = 1 << 40
ALPHABETS = {2: b"ab", 4: b"acgt", 26: bytes(range(0x61, 0x7B)), 256: bytes(range(256))}
LENGTHS = (1, 2, 31, 32, 33, 63, 64)
MAX_ERRORS = 8


def lower(b):
    """SX_SELECT_ASCII_NOCASE: 'A'..'Z' as 'a'..'z', no other byte (bytes.lower() touches ASCII only)"""
    return bytes(b).lower()


def last_row(pattern, texts, nocase=False):
    """min_j D[m][j] of Sellers' table for `pattern` over every text of `texts`: an int64 array"""
    if nocase:
        pattern, texts = lower(pattern), [lower(t) for t in texts]
    m, n = len(pattern), len(texts)
    assert m >= 1
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    lens = np.array([len(t) for t in texts], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(lens + 1)[:-1]])          # column 0 of every text
    total = int((lens + 1).sum())
    t = np.full(total, -1, dtype=np.int64)
    body = np.ones(total, dtype=bool)
    body[starts] = False
    t[body] = np.frombuffer(b"".join(texts), dtype=np.uint8)
    lift = np.arange(total, dtype=np.int64) + np.repeat(np.arange(n, dtype=np.int64), lens + 1) * BIG
    prev = np.zeros(total, dtype=np.int64)                              # row 0
    for i in range(1, m + 1):
        a = np.empty(total, dtype=np.int64)
        a[1:] = np.minimum(prev[:-1] + (t[1:] != pattern[i - 1]), prev[1:] + 1)
        a[starts] = i
        prev = np.minimum.accumulate(a - lift) + lift
    return np.minimum.reduceat(prev, starts)


def distance(pattern, text, nocase=False):
    """the least Levenshtein distance between `pattern` and a substring of `text`"""
    return int(last_row(pattern, [text], nocase)[0])


_memo = {}


def words(patterns, ks, strs, nocase=False):
    """the words of `strs` for the set (patterns, ks: an int or one per pattern), a uint64 array; memoised per distinct string"""
    patterns = [bytes(p) for p in patterns]
    ks = [ks] * len(patterns) if isinstance(ks, int) else list(ks)
    assert 1 <= len(patterns) == len(ks) <= 64 and all(0 <= k <= MAX_ERRORS and k < len(p) <= 64 for p, k in zip(patterns, ks))
    known = _memo.setdefault((tuple(patterns), tuple(ks), bool(nocase)), {})
    new = sorted({bytes(s) for s in strs} - set(known))
    if new:
        got = np.zeros(len(new), dtype=np.uint64)
        for p, (pattern, k) in enumerate(zip(patterns, ks)):
            got |= (last_row(pattern, new, nocase) <= k).astype(np.uint64) << np.uint64(p)
        known.update(zip(new, (int(w) for w in got)))
    return np.array([known[bytes(s)] for s in strs], dtype=np.uint64)


def word(patterns, ks, s, nocase=False):
    return int(words(patterns, ks, [s], nocase)[0])


# ---- planted patterns, texts and variants

def mix(x):
    """splitmix64's finaliser: a number from a place"""
    x = (x + 0x9E3779B97F4A7C15) & (1 << 64) - 1
    x = ((x ^ x >> 30) * 0xBF58476D1CE4E5B9) & (1 << 64) - 1
    x = ((x ^ x >> 27) * 0x94D049BB133111EB) & (1 << 64) - 1
    return x ^ x >> 31


def made(n, symbols, seed):
    """n bytes over ALPHABETS[symbols], a function of (n, symbols, seed)"""
    alphabet = ALPHABETS[symbols]
    return bytes(alphabet[mix(seed * 1000003 + i * 7 + n) % symbols] for i in range(n))


def legal_ks(length):
    return [k for k in range(MAX_ERRORS + 1) if k < length]


def edited(pattern, e, seed, kinds="sid"):
    """`pattern` with e edits at e different places, the first and the last byte among them where e >= 2 (seed picks which for e = 1):
    s a byte replaced by another value, i a byte put in behind the place, d the byte dropped.  The distance to the pattern is at most e"""
    m = len(pattern)
    assert 0 <= e <= m
    if e >= 2:
        places = [0, m - 1] + sorted(range(1, m - 1), key=lambda x: mix(seed * 64 + x))[:e - 2]
    else:
        places = [(0, m - 1)[seed % 2]][:e]
    out = []
    for at, x in enumerate(pattern):
        if at not in places:
            out.append(x)
            continue
        kind = kinds[mix(seed + at) % len(kinds)]
        other = (x + 1 + mix(seed + 5 * at) % 255) % 256 if len(set(pattern)) > 26 else [y for y in b"#%&0123456789" if y != x][mix(seed + at) % 12]
        if kind == "s":
            out.append(other)
        elif kind == "i":
            out += [x, other] if at < m - 1 else [other, x]      # (behind the last byte it would be no error: in front of it)
        # d: nothing
    return bytes(out)


def variant(pattern, e, seed=0, filler=b" ~ "):
    """(text, variant): a variant of `pattern` inside `filler`s whose distance to it by the TABLE is exactly e — edited() with the first
    seed for which that holds"""
    for s in range(seed, seed + 200):
        v = edited(pattern, e, s)
        text = filler + v + filler
        if distance(pattern, text) == e:
            return text, v
    raise AssertionError(("no variant at exactly", e, pattern))


def placed(v, where, n, seed):
    """a text of about n bytes of filler (upper-case letters and spaces, which no planted pattern holds) with v at its head, in its middle or as its tail"""
    fill = bytes(b"QWXZ JKVY"[mix(seed + i) % 9] for i in range(max(0, n - len(v))))
    cut = {"head": 0, "middle": len(fill) // 2, "tail": len(fill)}[where]
    return fill[:cut] + v + fill[cut:]


# ---- the lines of tests/test_gpu_fuzzy_device.py: printable text, 4 to 60 characters, one finding a line

WORDS = [b"password", b"administrator", b"login.example.com", b"kernel32.dll", "пароль".encode(), b"root", b"ssh-rsa", b"token",
         b"/etc/shadow", b"secret_key", b"BEGIN CERTIFICATE", b"cmd.exe"]
WORD_KS = [2, 2, 2, 1, 2, 1, 1, 1, 2, 2, 2, 1]
SHORT = b"passwo"      # len(WORDS[0]) - WORD_KS[0] bytes: the shortest string that can match WORDS[0]
FILL = [b"open", b"read", b"stat", b"mmap", b"conn", b"eth0", b"uid=10", b"/tmp/x", b"net:", b"0x7f", "мир".encode(), b"QWXZ"]


LONG_WORD = b"the quick brown fox jumps over a dog"      # 36 bytes: a set that holds it walks in 64-bit words
PLANTED, PLANTED_KS = WORDS + [LONG_WORD], WORD_KS + [3]


def many_classes():
    """64 patterns: three of WORDS, whose letters few pattern positions hold — the rarest classes —, and 61 of 64 bytes over 150 values
    that no line holds: more classes than the kernel keeps rows of in LDS, and the rows the three words need are among the others"""
    return WORDS[:3] + [bytes(0x80 + (p * 64 + i * 37 + p * p) % 120 if (p + i) % 5 else 1 + (p + i) % 30 for i in range(64)) for p in range(61)]


# the sets of tests/test_gpu_fuzzy_device.py: name -> (patterns, ks, nocase)
SETS = {
    "one": ([WORDS[0]], [2], False),
    "nine": (WORDS[:9], WORD_KS[:9], False),                                   # 32-bit words: a group of eight and one more
    "five": (WORDS[:4] + [LONG_WORD], WORD_KS[:4] + [3], False),               # 64-bit words: a group of four and one more
    "exact": ([WORDS[0], WORDS[3]], [0, 0], False),                            # k = 0: the substring selection
    "nocase": ([b"PASSWORD", b"begin certificate", "ПАРОЛЬ".encode(), b"Kernel32.DLL"], [2, 2, 2, 1], True),
    "sixty-four": ([FILL[i % 12][:2 + i % 3] + b"%d" % (i % 7) if i % 4 else PLANTED[i // 4 % 13] for i in range(63)] + [WORDS[0]],
                   [1 if i % 4 else PLANTED_KS[i // 4 % 13] for i in range(63)] + [1], False),
    "many": (many_classes(), [2, 2, 2] + [8] * 61, False),
}


def line(i, patterns=PLANTED, ks=PLANTED_KS):
    """line i: filler words with, in two lines of three, a variant of pattern i // 3 % n at 0 .. k + 1 errors at its head, in its middle
    or as its tail"""
    m = mix(i + 1)
    fill = [FILL[(m >> 8 * j) % len(FILL)] for j in range(1 + m % 3)]
    if i % 3 == 2:
        return b" ".join(fill + [b"%d" % (m % 9973)])
    p = i // 3 % len(patterns)
    e = (m >> 20) % (ks[p] + 2)
    if max(patterns[p]) < 0x80:
        v = edited(patterns[p], e, i)
        if (m >> 50) % 4 == 0:      # (one in four in the other case: what only a nocase set, or a fold in front, finds)
            v = v.swapcase()
    else:      # (a line is UTF-8: whole characters are replaced, each an error or two)
        chars = list(patterns[p].decode())
        for j in range((e + 1) // 2):
            chars[(m >> 30 + j) % len(chars)] = "жё"[j % 2]
        v = "".join(chars).encode()
    if len(v) > 30:
        fill = fill[:1]
    at = (0, len(fill) // 2 + 1, len(fill))[(m >> 40) % 3]
    return b" ".join(fill[:at] + [v] + fill[at:])


MERGED_LINES = 1600      # under `-e ascii -e utf-8`: more than three parts of 1024 findings


def lines(n, patterns=PLANTED, ks=PLANTED_KS):
    """n lines; the first four are SHORT, SHORT without its last byte, an exact word and a line that holds none"""
    head = [SHORT, SHORT[:-1], WORDS[0], b"nothing here"]
    out = (head + [line(i, patterns, ks) for i in range(n)])[:n]
    assert all(4 <= len(x.decode()) <= 60 and b"\n" not in x for x in out)
    return out


def trip_lines(r):
    """r + 1 lines of few distinct values: line 0 holds WORDS[0] exactly, line r — the lane that had record 0, a trip later — holds
    a prefix of it that is one error too far (so a lane that kept record 0's columns or its bits would say yes)"""
    few = [WORDS[0] + b" at the head", b"open read stat", b"eth0 passw0rd conn", b"mmap", b"nothing of it here", b"root and t0ken", b"uid=10 /tmp/x"]
    out = [few[i % len(few)] for i in range(r)]
    out[0] = few[0]
    return out + [WORDS[0][:len(WORDS[0]) - WORD_KS[0] - 1] + b" the rest is missing"]


LONG_TAIL = "\U0001F600\U0001F4A9".encode()      # long_plant.LIMIT_NEEDLE: the last eight bytes of limit_lines()'s long lines
LONG_SET = ([LONG_TAIL, b"limit last line", b"between the twa", LONG_TAIL[4:] + LONG_TAIL[:4]], [1, 2, 1, 0])
