"""A planted buffer whose findings are known line by line, for the kernels that work on a result lying in HBM (tests/test_result_plant.py
on the CPU; tests/test_gpu_result_strides.py and tests/test_gpu_result_edges.py on the device).  The buffer is ASCII lines separated by
`\\n`, every line 4 to 60 bytes of printable ASCII: at least chars_min, and below the default output line length, so that a line is
never cut.  With `-e ascii -n 4` (MS1) line k is finding k; with `-e ascii -e utf-8 -n 4` (MS2) every line is found once by each
Mission, in line order within a Mission.  Everything here is a function of the line number: no random state.

What the lines hold makes every operation's answer depend on records everywhere, so that a record skipped, repeated or shifted changes
the answer:

 duplicates  two lines of three repeat an earlier line, a few lines or anywhere back: classes of size 1, 2 and 3 or more.  DOMINANT is
             planted thousands of times: in runs of 3 neighbours every 128 lines, in runs of 70 (longer than a wavefront) every 65536
             lines, and scattered.
 the fold    one line of 41 is the upper case of an earlier line: ignore_case joins classes that the plain comparison keeps apart.
 tokens      the six KINDs (a sixth of the lines each), `key=` and `/tmp` in the padding, the hexadecimal payload: spread evenly.
 prefix and suffix tokens   `-> ` stands only at the beginning of a line (one line of four), ` ;;` only at the end (one of five).

prefix(k) is the first k - 1 lines and then SENTINEL, which matches every pattern the tests use (predicates()), equals line 0 byte for
byte and line 1 under the fold: with MS1 a prefix has exactly k findings, and its last record is a positive and, for k >= 2, a duplicate.

expected(ms, data) is the only source of expected findings: the rows of the oracle's text."""
import re

import numpy as np

import refconfig as rc
import sxo_binding as sxo

P = 16777213                     # a prime below 2^24: k -> k * 2654435761 % P is one to one below P
KIND = [b"open", b"read", b"stat", b"exec", b"mmap", b"conn"]
PAD = b" key=41 /tmp/cache.d/net:eth0 uid=1000 key=7 /var/log/syslog.1 pid=311 tmp=/tmp/x mode=0644 "
SENTINEL = b"-> mmap:c0ffee key=77777 /tmp/x uid=10 /var/log ;;"
DOMINANT = b"stat:7e57ed /var/log/syslog.1 key=41"
OUTPUT_BOM = b"\xef\xbb\xbf"
PRECISION_CODE = {b"<": 0, b" ": 1, b">": 2}       # Before, Exact, After: sx_finding's precision

# the predicates of the GPU tests; SENTINEL holds every one of them, and each selects 5 % to 60 % of the lines
SUBSTRING = b"mmap"
SIXTEEN = [b"e5c", b"a7:", b"3f0", b"0c4", b"9b", b"d1", b"77", b"6a0", b"f2", b"48", b"1e", b"b3", b"c0ffee", b"5d", b"82", b"uid=10"]
NOCASE = b"Key=7"
REGEXES = [rb"^-> [a-z]+:", rb"[^0-9] ;;$", rb"mmap:[0-9a-f]+"]
EXTRACTS = [rb"[0-9]{5,}", rb"uid="]                  # (runs of one class and a literal: leftmost-first is leftmost-longest)
LABELS = [rb"^-> ", rb";;$", rb"mmap", rb"[0-9]{4}", rb"^.{40,}$", rb"key=7"]


def ms1():
    return rc.missions(encodings=["ascii"], chars_min="4")


def ms2():
    return rc.missions(encodings=["ascii", "utf-8"], chars_min="4")


def mix(k):
    return k * 2654435761 % P


def fresh(j):
    """the j-th line that is no copy: lower case letters, digits and punctuation only (its upper case is another string)"""
    if j % 29 == 11:
        return b"i=%x" % j                                                # the short ones: 4 bytes and a little more
    body = b"%s:%06x" % (KIND[j // 3 % 6], mix(j))
    head = b"-> " if j % 4 == 1 else b""
    tail = b" ;;" if j % 5 == 2 else b""
    at, n = j * 13 % 40, j * 7 % 44                                       # at most 3 + 11 + 43 + 3 = 60 bytes
    return head + body + PAD[at:at + n] + tail


_lines = []


def lines(n):
    """the first n lines"""
    out = _lines
    if not out:
        out += [SENTINEL, SENTINEL.upper(), DOMINANT]
    for k in range(len(out), n):
        if k % 128 in (5, 6, 7) or k % 65536 < 70 or k % 251 == 17:
            line = DOMINANT
        elif k % 41 == 13:
            line = out[mix(k) % k].upper()
        elif k % 3 == 1:
            line = out[k - 1 - mix(k) % min(k, 3000)]              # a neighbour, or some thousand lines back
        elif k % 3 == 2:
            line = out[mix(k) // 7 % k]                                   # anywhere in front
        else:
            line = fresh(k)
        out.append(line)
    return out[:n]


def buffer(n):
    """n lines"""
    return b"\n".join(lines(n)) + b"\n"


def prefix(k):
    """the first k - 1 lines, then SENTINEL"""
    assert k >= 1
    return b"\n".join(lines(k - 1) + [SENTINEL]) + b"\n"


def with_token(n, k, token=b"{pick}"):
    """n lines of which exactly k, spread over the buffer, hold `token` (which stands nowhere else) in their middle: they keep their
    beginning and their end, with the prefix and suffix tokens, and are still 60 bytes at most"""
    assert 0 < k <= n
    out = lines(n)
    at = sorted({i * n // k for i in range(k)})
    assert len(at) == k
    for i in at:
        assert token not in out[i]
        half, most = len(out[i]) // 2, (60 - len(token)) // 2
        out[i] = out[i][:half][:most] + token + out[i][half:][-most:]
    return b"\n".join(out) + b"\n"


class Rows:
    """the oracle's rows as arrays — position, precision (sx_finding's code), completes, mission (the label's letter), length —, their
    strings `strs` and their text `raw` (a row of the oracle's output without its leading \\n); `uniq` / `inv`: strs[i] == uniq[inv[i]],
    uniq in the order of the first occurrence, so that a predicate is evaluated once per different string"""

    def __init__(self, rows, raw):
        self.rows, self.raw, self.n = rows, raw, len(rows)
        self.position = np.array([r[0] for r in rows], dtype=np.uint64)
        self.precision = np.array([PRECISION_CODE[r[1][:1]] for r in rows], dtype=np.uint8)
        self.completes = np.array([r[1][1:] == b"+" for r in rows], dtype=bool)
        self.mission = np.array([r[2][1] - 97 if r[2] else 0 for r in rows], dtype=np.uint8)
        self.strs = [r[3] for r in rows]
        self.length = np.array([len(s) for s in self.strs], dtype=np.uint64)
        self._classes = None

    @property
    def uniq(self):
        self._classes = self._classes or classes(self.strs)
        return self._classes[0]

    @property
    def inv(self):
        self._classes = self._classes or classes(self.strs)
        return self._classes[1]

    def mask(self, pred):
        """pred(string) per row, as a bool array"""
        return np.array([bool(pred(u)) for u in self.uniq], dtype=bool)[self.inv]

    def take(self, index, strs=None):
        """the rows mask keeps (a bool array), or the rows index names (an int array: a row may come several times), with other
        strings if `strs` is given"""
        index = np.nonzero(index)[0] if index.dtype == bool else index
        out = Rows.__new__(Rows)
        out.rows, out.n, out._classes = None, len(index), None
        out.position, out.precision, out.completes, out.mission = self.position[index], self.precision[index], self.completes[index], self.mission[index]
        where = index.tolist()
        out.raw = [self.raw[i] for i in where] if strs is None else None
        out.strs = [self.strs[i] for i in where] if strs is None else strs
        out.length = self.length[index] if strs is None else np.array([len(s) for s in strs], dtype=np.uint64)
        return out

    def text(self):
        """the oracle's output for these rows"""
        return OUTPUT_BOM + b"".join(b"\n" + r for r in self.raw) + b"\n"


def classes(keys):
    """(the different keys in the order of their first occurrence, per key the index of its class)"""
    ids = {}
    inv = np.array([ids.setdefault(k, len(ids)) for k in keys], dtype=np.int64)
    return list(ids), inv


_expected = {}


def parse(text, several):
    """the rows of the oracle's text with --radix=x: [(position, precision mark and continuation mark, Mission label or b"", string)], and the rows as they are printed"""
    assert text.startswith(OUTPUT_BOM) and text.endswith(b"\n")
    rows, raw = [], text[len(OUTPUT_BOM):-1].split(b"\n")[1:]
    for row in raw:
        head, rest = row.split(b"\t", 1)
        label = b""
        if several:
            label, rest = rest.split(b"\t", 1)
            assert label[:1] == b"(" and label[-1:] == b")"
        rows.append((int(head[1:-1], 16), head[:1] + head[-1:], label, rest))
    return rows, raw


def oracle_text(ms, data):
    return sxo.run_cli(ms, [data], radix="x")


def expected(ms, data):
    """the oracle's findings of `data`: a Rows (cached by every field of every Mission and the data)"""
    key = (tuple(tuple(sorted(m.items())) for m in ms), len(data), hash(data))
    if key not in _expected:
        _expected[key] = Rows(*parse(oracle_text(ms, data), len(ms) > 1))
    return _expected[key]


def to_python(pattern):
    """a pattern of the library's regex language for Python's re: `$` is the end of the string, not the place in front of a last \\n"""
    return re.compile(pattern.replace(b"$", rb"\Z"))


def predicates():
    """{name: string -> bool}: what the GPU tests select by, for the plant's own test of their shares"""
    rx = [to_python(p) for p in REGEXES]
    lab = [to_python(p) for p in LABELS]
    ext = [to_python(p) for p in EXTRACTS]
    out = {"substring": lambda s: SUBSTRING in s, "sixteen": lambda s: any(p in s for p in SIXTEEN), "nocase": lambda s: NOCASE.lower() in s.lower(),
           "regexes": lambda s: any(r.search(s) for r in rx), "extracts": lambda s: any(r.search(s) for r in ext)}
    for k, r in enumerate(rx):
        out["regex %d" % k] = r.search
    for k, r in enumerate(lab):
        out["label %d" % k] = r.search
    return out


# ---- the keyword lists of the GPU tests, and plain models of the operations over a Rows' strings ----

def keyword_list():
    """about 2000 keywords of 4 bytes or more for a PatternSet: a few dozen that occur — rare ones, a kind with the head of its payload,
    DOMINANT's and SENTINEL's payloads — among decoys that cannot (a payload is never followed by `;`)"""
    occur = [b"%s:%02x" % (KIND[i % 6], mix(i) % 256) for i in range(30)] + [b"-> exec", b"read:1", b"conn:f", b"c0ffee", b"stat:7e57ed", b"/var/log/sys"]
    decoys = [b"%06x;%s" % (mix(i + 1), KIND[i % 6]) for i in range(2000 - len(occur))]
    return decoys[:700] + occur + decoys[700:]


HOT_SHORT, HOT_LONG = b":", DOMINANT      # a keyword that ends in an early state and one that ends in the last: both stand in thousands of lines


def tally_list():
    """more unique keywords than the tally kernel counts in LDS (4096 ids, numbered in the order of the states the keywords end in, so
    the short ones are counted there), with a hot one on either side: HOT_SHORT in nearly every line, HOT_LONG = DOMINANT, the longest,
    in every line that is DOMINANT; `77` and `777` stand at overlapping places in SENTINEL's 77777"""
    decoys = [b"%06x;%s" % (mix(i + 1), KIND[i % 6]) for i in range(4200)]
    return decoys[:1500] + [HOT_SHORT, b"77", b"777", b"c0ffee"] + [b"%s:%02x" % (KIND[i % 6], mix(i) % 256) for i in range(30)] + decoys[1500:] + [HOT_LONG]


def occurrences(uniq, keywords):
    """per keyword {index into uniq: at how many places of that string the keyword stands} — overlapping places count, as
    sx_result_tally_device counts them —: bytes.startswith at every place where the keyword's first four bytes stand (found with
    numpy over the joined strings), and bytes.find from one place behind the last hit for keywords shorter than that"""
    joined = b"\n".join(uniq) + b"\n\n\n\n"
    a = np.frombuffer(joined, dtype=np.uint8).astype(np.uint32)
    starts = np.cumsum([0] + [len(u) + 1 for u in uniq[:-1]])
    w4 = a[:-3] | a[1:-2] << 8 | a[2:-1] << 16 | a[3:] << 24
    out, by_head = [dict() for _ in keywords], {}
    for k, p in enumerate(keywords):
        assert p and b"\n" not in p
        if len(p) >= 4:
            by_head.setdefault(int.from_bytes(p[:4], "little"), []).append(k)
    cand = np.nonzero(np.isin(w4, np.array(list(by_head), dtype=np.uint32)))[0]
    owner = np.searchsorted(starts, cand, side="right") - 1
    for at, head, u in zip(cand.tolist(), w4[cand].tolist(), owner.tolist()):
        for k in by_head[head]:
            if joined.startswith(keywords[k], at):          # (a keyword holds no \n: it lies inside string u)
                out[k][u] = out[k].get(u, 0) + 1
    for k, p in enumerate(keywords):
        if len(p) < 4:
            for u, s in enumerate(uniq):
                o, c = s.find(p), 0
                while o >= 0:
                    c, o = c + 1, s.find(p, o + 1)
                if c:
                    out[k][u] = c
    return out


def held_by_any(rows, occ):
    """the rows whose string holds one of the keywords, as a bool array (occ: occurrences(rows.uniq, keywords))"""
    m = np.zeros(len(rows.uniq), dtype=bool)
    for d in occ:
        m[list(d)] = True
    return m[rows.inv]


def first_index(rows):
    """per class the index of its first row"""
    return np.unique(rows.inv, return_index=True)[1]


def tally_model(rows, occ, never, base=0):
    """(hits, first) per keyword as sx_tally_set_read returns them"""
    mult, first = np.bincount(rows.inv, minlength=len(rows.uniq)), first_index(rows)
    hits = [sum(c * int(mult[u]) for u, c in d.items()) for d in occ]
    return hits, [base + min(int(first[u]) for u in d) if d else never for d in occ]


def distinct_model(strs, first_bit, repeated_bit, shift, nocase=False):
    """(the words of sx_result_distinct_device in print order as a uint64 array, its info's counted fields, the classes' keys, per row
    its class): bytes.lower() folds 'A'..'Z' and nothing else"""
    keys, inv = classes([s.lower() for s in strs] if nocase else strs)
    size = np.bincount(inv, minlength=len(keys)).astype(np.uint64)
    words = np.minimum(size, np.uint64(0xFFFFFFFF))[inv] << np.uint64(shift) | np.where(size[inv] > 1, np.uint64(repeated_bit), np.uint64(0))
    words[np.unique(inv, return_index=True)[1]] |= np.uint64(first_bit)
    return words, dict(findings=len(strs), distinct=len(keys), repeated=int((size > 1).sum())), keys, inv
