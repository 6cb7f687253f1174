"""Test helper: planted inputs for what lies between the scan kernels and stage B (stringsext_amd/csrc/sx_sort.hip): the pack of the
per-sub-chunk record regions, the sort and join of records into runs, and the interleave of the Missions' findings.

No plant probes classification: every string is made of characters any classifier finds (letters; letters and two-byte characters of one
block), strings are separated by NUL and the background is zero.  What varies is WHERE records land and HOW MANY there are.

Stage A plants (1 KiB sub-chunks).  A record is one stretch inside one sub-chunk: a closed stretch of at least min_chars characters, or a
piece that is open — one that continues a stretch of the sub-chunk in front, or one that reaches the sub-chunk's (or the input's) last
byte — whatever its length.  records_per_region() is that model; a Plant carries the data, the runs (start, end, chars) it planted and
notes (position, what) for a failing assertion's message.

    counts       region w holds c(w) closed strings a few bytes apart, c cycling through the pack lanes' and the region's edges
    join         threshold splits over a sub-chunk edge, neighbours that touch but do not continue, chains over hundreds of sub-chunks
    second_trip  one region more than region_sum_scan_kernel's loop handles in one trip
    key_width    lengths around a power of two, runs at every power of two below

Interleave plants: Mission sets in the per-encoding form of the command line, UTF-8 Missions of one block each with the ASCII filter off,
whose lists are disjoint; the same flags twice give lists that tie at every position.  Everything is deterministic: no random numbers."""
import glob
import os
import re
from collections import namedtuple

SUB = 1024                  # the sub-chunk size every stage A plant is made for
SLICE = 4096                # the reference's input slice: where the merger's parts are cut
LETTERS = "abcdefghijklmnopqrstuvwxyz"
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stringsext_amd", "csrc")

Plant = namedtuple("Plant", "data runs notes")


# ---- constants the sizes depend on, from the sources ----

def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constant(name):
    """`constexpr <integer type> name = N;` from the sources: a constant that is gone or spelt otherwise fails the tests, it does not
    quietly move them off the edge"""
    found = set()
    for path in sorted(glob.glob(os.path.join(CSRC, "*.h*"))):
        found |= {int(v) for v in re.findall(r"constexpr\s+(?:uint32_t|u32|int)\s+%s\s*=\s*(\d+)u?\s*;" % name, _source(path))}
    assert len(found) == 1, (name, found)
    return found.pop()


def sum_scan_trip():
    """the block sums one trip of region_sum_scan_kernel's loop handles"""
    body = re.search(r"void region_sum_scan_kernel\(.*?\n}\n", _source("sx_sort.hip"), re.S).group(0)
    step = set(re.findall(r"for \(uint32_t base = 0; base < n_blocks; base \+= (\d+)\)", body))
    assert len(step) == 1 and "__launch_bounds__(%s) void region_sum_scan_kernel" % next(iter(step)) in _source("sx_sort.hip"), step
    return int(step.pop())


def default_region_cap():
    """the record slots of a region when SX_REGION_CAP is unset (sx_ctx.hpp)"""
    found = set(re.findall(r"uint32_t\s+region_cap\s*=\s*([1-9]\d*)\s*;", _source("sx_ctx.hpp")))
    assert len(found) == 1, found
    return int(found.pop())


# ---- strings ----

def text(i, two_byte):
    """string number i -> (bytes, characters): 4 + i % 4 characters, so that a key moved with another record's payload shows; two_byte:
    every other character is one of U+0410 .. U+042F (inside -u Cyrillic), so that chars != len"""
    k = 4 + i % 4
    if two_byte:
        s = "".join(LETTERS[(i * 7 + j) % 26] if j % 2 == 0 else chr(0x0410 + (i + j) % 32) for j in range(k))
    else:
        s = "".join(LETTERS[(i * 7 + j) % 26] for j in range(k))
    return s.encode("utf-8"), k


def chain_text(i, chars, two_byte):
    """a long stretch: letters, or (two_byte) two-byte characters with a letter every 97th — an odd run in between, so the characters
    straddle sub-chunk edges at both phases"""
    if two_byte:
        s = "".join(LETTERS[(i + j) % 26] if j % 97 == 0 else chr(0x0410 + (i + j) % 32) for j in range(chars))
    else:
        s = "".join(LETTERS[(i + j) % 26] for j in range(chars))
    return s.encode("utf-8")


ASCII_FLAGS = dict(encodings=["ascii,4"])                                                      # the per-Mission kernel's Emitter
FUSED_FLAGS = dict(encodings=["utf-8"], chars_min="4", unicode_block_filter="Cyrillic")       # fused_atlas.set_flags("u8", ("u8", 4, "Cyrillic"))


def records_per_region(runs, length, min_chars, sub=SUB):
    """the model: per sub-chunk the closed stretches of at least min_chars characters plus the open pieces, of `runs` (every stretch of
    the input, whatever its length)"""
    counts = [0] * ((length + sub - 1) // sub)
    for s, e, chars in runs:
        for w in range(s // sub, (e - 1) // sub + 1):
            lo, hi = max(s, w * sub), min(e, (w + 1) * sub)
            is_open = lo > s or hi == min((w + 1) * sub, length)
            if is_open or chars >= min_chars:
                counts[w] += 1
    return counts


def kept(runs, min_chars):
    return [r for r in runs if r[2] >= min_chars]


def describe(plant, pos):
    """the last note at or in front of byte `pos`"""
    best = None
    for p, what in plant.notes:
        if p <= pos:
            best = (p, what)
    return best


def first_difference(plant, got, want):
    """-> None if equal, else the first run that differs and what the plant put there"""
    if got == want:
        return None
    k = 0
    while k < len(got) and k < len(want) and got[k] == want[k]:
        k += 1
    g = got[k] if k < len(got) else None
    w = want[k] if k < len(want) else None
    pos = (w or g)[0]
    return dict(index=k, got=g, want=w, region=pos // SUB, byte_in_region=pos % SUB, planted=describe(plant, pos))


class _Builder:
    def __init__(self, two_byte):
        self.two, self.d, self.runs, self.notes, self.i = two_byte, bytearray(), [], [], 0

    def put(self, pos, s, chars, what):
        """a stretch at `pos`; it must not touch what is there"""
        if len(self.d) < pos + len(s) + 1:
            self.d += bytes(pos + len(s) + 1 - len(self.d))
        assert pos >= 0 and not any(self.d[max(pos - 1, 0):pos + len(s) + 1]), (pos, what)
        self.d[pos:pos + len(s)] = s
        self.runs.append((pos, pos + len(s), chars))
        self.notes.append((pos, what))
        return pos + len(s)

    def string(self, pos, what):
        s, k = text(self.i, self.two)
        self.i += 1
        return self.put(pos, s, k, what)

    def strings(self, pos, n, what):
        """n strings back to back, one NUL apart"""
        for _ in range(n):
            pos = self.string(pos, what) + 1
        return pos

    def split(self, edge, before, after, what):
        """a stretch of before + after characters whose character number `before` begins at `edge`"""
        width = 2 if self.two else 1
        s = chain_text(self.i, before + after, False)
        if self.two:
            s = "".join(chr(0x0410 + (self.i + j) % 32) for j in range(before + after)).encode("utf-8")
        self.i += 1
        return self.put(edge - before * width, s, before + after, what)

    def next_edge(self, at_least):
        return (max(len(self.d), at_least) + SUB - 1) // SUB * SUB + SUB

    def plant(self, length=None):
        data = bytes(self.d) if length is None else bytes(self.d[:length]) + bytes(max(0, length - len(self.d)))
        return Plant(data, sorted(self.runs), sorted(self.notes))


# ---- 1. counts ----

def count_cycle():
    lanes, cap = constant("kPackLanes"), default_region_cap()
    return (0, 1, 2, lanes - 1, lanes, lanes + 1, 31, 32, 33, 47, 48, 49, cap - 1, cap)


def counts_sizes():
    per = constant("kScanPerBlock")
    return (1, 3, per - 1, per, per + 1, 2 * per + 1, 4 * per + 3)


def counts_plant(n_regions, two_byte, raised=None):
    """-> (Plant, counts): region w holds c(w) closed strings 5 to 8 (two_byte: 7 to 11) bytes apart — several inside one lane's 16
    bytes —, c cycling through count_cycle(); region `raised` holds one more than a region's slots; the input ends inside its last region"""
    cyc, cap = count_cycle(), default_region_cap()
    b = _Builder(two_byte)
    counts = []
    for w in range(n_regions):
        c = cap + 1 if w == raised else cyc[w % len(cyc)]
        end = b.strings(w * SUB + 1 + w % 5, c, "region %d: %d strings" % (w, c))
        assert end < (w + 1) * SUB
        counts.append(c)
    length = max(len(b.d) + 2, (n_regions - 1) * SUB + 7)
    assert (n_regions - 1) * SUB < length < n_regions * SUB
    return b.plant(length), counts


def sparse_plant(n_regions, two_byte):
    """a string in every 7th region: far fewer than a quarter of the default slots"""
    b = _Builder(two_byte)
    for w in range(0, n_regions, 7):
        b.string(w * SUB + 33, "region %d: one string" % w)
    return b.plant((n_regions - 1) * SUB + 7 if n_regions > 1 else 64)


# ---- 2. join ----

JOIN_THRESHOLDS = (4, 7)
JOIN_CHAINS = (1, 2, 3, 65, 257, 600)
JOIN_ENDINGS = ("lone", "chain_tail", "open_short", "multiple")


def join_plant(two_byte, ending="lone"):
    """about 1 MiB; see the module's text and the notes of every stretch"""
    b = _Builder(two_byte)
    width = 2 if two_byte else 1
    # the buffer begins inside a string: record 0 is open at its start
    b.put(0, chain_text(3, 9, two_byte), 9, "the input begins inside a string")
    b.strings(40, 30, "filler")
    for n in JOIN_THRESHOLDS:
        for keep in (0, 1):
            for i in range(1, n):
                e = b.next_edge(0)
                b.strings(e - SUB + 16, 48, "filler")
                b.split(e, i, n - 1 - i + keep, "threshold %d: %d + %d characters over edge %d: %s" % (n, i, n - 1 - i + keep, e, "kept" if keep else "dropped"))
    for n in (5, 9):
        # touch but do not continue: a run whose last byte is the edge's last byte, a NUL first in the next sub-chunk, a new run at edge + 1
        e = b.next_edge(0)
        b.split(e, n, 0, "ends with edge %d's last byte; nothing continues it" % e)
        b.split(e + 1, 0, n, "begins at edge + 1 behind a NUL at the edge")
        b.strings(e + 40, 25, "filler")
        # the mirror image: a NUL as the edge's last byte, a run that begins exactly at the edge
        e = b.next_edge(0)
        b.split(e - 1, n, 0, "ends one byte in front of edge %d's last byte" % e)
        b.split(e, 0, n, "begins exactly at edge %d behind a NUL" % e)
        # ... and short ones (below either threshold) at both places: open pieces are records whatever their length
        e = b.next_edge(0)
        b.split(e, 3, 0, "3 characters ending with edge %d's last byte" % e)
        b.split(e + 1 + SUB, 0, 3, "3 characters, closed")
    if two_byte:
        # a character whose first byte is an edge's last byte: inside a stretch, as its first and as its last character
        for lead, tail in ((3, 3), (0, 6), (6, 0), (1, 1)):
            e = b.next_edge(0)
            s = chain_text(b.i, lead + 1 + tail, False).decode()
            s = s[:lead] + "Ж" + s[lead + 1:]
            b.i += 1
            b.put(e - 1 - lead, s.encode("utf-8"), lead + 1 + tail, "a two-byte character over edge %d, %d characters in front, %d behind" % (e, lead, tail))
    for _ in range(12):
        b.strings(b.next_edge(0) + 5, 60, "a region with 60 strings")
    for k in JOIN_CHAINS:
        e = b.next_edge(0)
        head, tail = 3 + k % 5, 2 + k % 3
        chars = (k * SUB) // width + head + tail
        s = chain_text(b.i, chars, two_byte)
        if two_byte:    # (a letter every 97th character: as many bytes as the other variant's chain has, cut at a character)
            s = chain_text(b.i, 2 * chars, True)[:k * SUB + (head + tail) * width].decode("utf-8", "ignore").encode("utf-8")
            chars = len(s.decode("utf-8"))
        b.i += 1
        start = e - head * width - (1 if two_byte and k % 2 else 0)
        end = b.put(start, s, chars, "a chain over %d whole sub-chunks from edge %d" % (k, e))
        assert (end - 1) // SUB - start // SUB >= k + 1
        b.strings(end + 1, 12, "filler behind a chain")
    e = b.next_edge(0)
    if ending == "lone":
        end = b.string(e + 100, "the input ends in a kept lone run")
        return b.plant(end)
    if ending == "chain_tail":
        s = chain_text(b.i, (2 * SUB) // width + 40, two_byte)
        end = b.put(e - 10 * width, s, (2 * SUB) // width + 40, "the input ends in the tail piece of a chain")
        assert end % SUB
        return b.plant(end)
    if ending == "open_short":
        end = b.split(e, 1, 2, "the input ends in an open piece whose chain stays below the threshold")
        return b.plant(end)
    assert ending == "multiple"
    end = b.split(e + SUB, 6, 0, "a run that reaches the input's end, a multiple of the sub-chunk")
    assert end % SUB == 0
    return b.plant(end)


# ---- 3. second_trip ----

def second_trip_plant():
    """one string in every 61st region; the regions around the end of region_sum_scan_kernel's first trip hold 3, cap and 2 strings, the
    last one 1.  -> (Plant, counts) with counts a dict of the regions that hold anything"""
    trip = sum_scan_trip() * constant("kScanPerBlock")
    n_regions, cap = trip + 5, default_region_cap()
    special = {trip - 1: 3, trip: cap, trip + 1: 2, n_regions - 1: 1}
    data = bytearray(n_regions * SUB)
    runs, notes, counts, i = [], [], {}, 0
    for w in sorted(set(range(0, n_regions, 61)) | set(special)):
        c = special.get(w, 1)
        pos = w * SUB + 1 + w % 7
        notes.append((pos, "region %d: %d strings" % (w, c)))
        for _ in range(c):
            s, k = text(i, False)
            data[pos:pos + len(s)] = s
            runs.append((pos, pos + len(s), k))
            pos += len(s) + 1
            i += 1
        counts[w] = c
    length = runs[-1][1] + 2
    assert (n_regions - 1) * SUB < length < n_regions * SUB
    del data[length:]
    return Plant(data, runs, notes), counts


# ---- 4. key_width ----

KEY_WIDTH_K = (16, 20)


def key_width_lengths():
    return [(1 << k) + d for k in KEY_WIDTH_K for d in (-1, 0, 1)]


def key_width_plant(length, dense, two_byte=False):
    """runs at offset 0, at length - 4 (two_byte: - 8; ending with the input) and over 2^j for every j whose 2^j lies inside the input,
    from 2^0 on; dense: 40 more strings in region 3, enough to overflow regions of 2 slots — and to leave unused slots in the large
    regions that follow"""
    b = _Builder(two_byte)
    width = 2 if two_byte else 1
    end = b.split(0, 0, 5, "a run at offset 0 (over 1, 2 and 4; two_byte: and 8)")
    if dense:
        b.strings(3 * SUB + 40, 40, "region 3: 40 strings")
    j = 3
    while (1 << j) + 4 * width < length - 8 * width:
        if (1 << j) > end:
            before = min(2 + j % 3, ((1 << j) - end - 1) // width) if j < 5 else 2 + j % 3     # (the first ones lie close together)
            end = b.split(1 << j, before, 3 + j % 2, "a run over 2^%d" % j)
        j += 1
    b.split(length - 4 * width, 0, 4, "a run that ends with the input")
    return b.plant(length)


# ---- the timing lines (SX_TIMING: one per Mission and stage A call, one per device merge) ----

def stage_a_lines(err):
    """[(mission, words)] of the stage A lines in what SX_TIMING wrote"""
    return [(int(m.group(1)), m.group(0)) for m in re.finditer(r"\[sx\] mission (\d+): kernel [^\n]* runs", err)]


def merge_lines(err):
    """[(missions, findings, parts)] of the device merges"""
    return [tuple(int(v) for v in m.groups())
            for m in re.finditer(r"\[sx\] device merge of (\d+) missions \(\d+ held back on the device\): (\d+) findings, (\d+) parts", err)]


# ---- interleave ----

BLOCKS = {"ascii": None, "Cyrillic": 0x0416, "Greek": 0x03B1, "Hebrew": 0x05D0, "Arabic": 0x0627}
SINGLE_BYTE = ["koi8-r,4", "windows-1251,4", "iso-8859-5,4", "ibm866,4", "windows-1252,4"]


def mission_flag(kind):
    return "ascii,4" if kind == "ascii" else "utf-8,4,None,%s" % kind


def block_text(kind, i):
    """finding number i of a Mission of `kind`: 4 + i % 4 characters of its block"""
    k = 4 + i % 4
    if kind == "ascii":
        return "".join(LETTERS[(i * 7 + j) % 26] for j in range(k)).encode()
    return "".join(chr(BLOCKS[kind] + (i + 3 * j) % 16) for j in range(k)).encode("utf-8")


Interleave = namedtuple("Interleave", "name flags data host_way")


def _lay(length, placed):
    """placed: [(position, kind)] at least 16 bytes apart"""
    data = bytearray(length)
    last = -16
    for i, (pos, kind) in enumerate(sorted(placed)):
        s = block_text(kind, i)
        assert pos >= last + 16 and pos + len(s) < length, (pos, kind)
        data[pos:pos + len(s)] = s
        last = pos
    return bytes(data)


def grid(kind, first, step, n):
    return [(first + step * k, kind) for k in range(n)]


INTERLEAVE_TOTALS = (1, 63, 64, 65, 129)
_interleave = {}


def interleave_plants():
    """-> {name: Interleave}.  host_way: the plant has at least 4096 findings in two lists or more (test_record_plant.py asserts it on
    the oracle's output), so a Scanner without result_on_device interleaves it on the device too"""
    out = _interleave
    if out:
        return out

    def add(name, kinds, data, host_way):
        out[name] = Interleave(name, [mission_flag(k) for k in kinds], data, host_way)
    # every list tied with a twin (4 Missions); the same with a fifth that ties with nobody
    body = grid("Cyrillic", 0, 64, 1500) + grid("Greek", 32, 64, 1500)
    add("twins4", ["Cyrillic", "Greek", "Cyrillic", "Greek"], _lay(100 * 1024, body), True)
    add("twins5", ["Cyrillic", "Greek", "ascii", "Cyrillic", "Greek"], _lay(100 * 1024, body + grid("ascii", 16, 128, 700)), True)
    # one Mission with no findings, first, in the middle and last
    body = grid("ascii", 0, 48, 3000) + grid("Cyrillic", 16, 96, 1500)
    for at in (0, 1, 2):
        kinds = ["ascii", "Cyrillic"]
        kinds.insert(at, "Hebrew")
        add("empty%d" % at, kinds, _lay(150 * 1024, body), True)
    # one Mission whose findings all precede everybody else's, one whose findings all follow
    body = grid("Greek", 0, 32, 1000) + grid("ascii", 40000, 64, 2000) + grid("Cyrillic", 40016, 64, 2000) + grid("Hebrew", 200000, 32, 1000)
    add("apart", ["Hebrew", "ascii", "Greek", "Cyrillic"], _lay(240 * 1024, body), True)
    # thousands of findings inside one tile of the position range, which a single far outlier of another Mission stretches
    body = grid("ascii", 1 << 20, 32, 5000) + grid("Cyrillic", (1 << 20) + 16, 320, 300) + [((16 << 20) - 64, "Greek")]
    add("one_tile", ["Greek", "ascii", "Cyrillic"], _lay(16 << 20, body), True)
    # (the outlier in front: for a result kept on the device only — the device replay hands the run at the buffer's very beginning to
    # the host, a list that is not in HBM when the merge begins goes to the host's interleave, and only a result that is to stay on
    # the device has such a list uploaded first)
    add("one_tile_first", ["ascii", "Cyrillic", "Greek"], _lay(16 << 20, [(64, "Greek")] + [(p + (14 << 20), k) for p, k in body[:-1]]), False)
    # totals of 1, 63, 64, 65 and 129 findings over all four lists, the twin's included (a Cyrillic string counts twice): the merger's
    # n / 64 tiles are 0 (one tile at least), 0, 1, 1 and 2
    for total in INTERLEAVE_TOTALS:
        a = total // 4
        body = grid("ascii", 4096, 64, total - 3 * a) + grid("Cyrillic", 4096 + 16, 64, a) + grid("Greek", 4096 + 32, 64, a)
        add("total%d" % total, ["Cyrillic", "ascii", "Greek", "Cyrillic"], _lay(64 * 1024, body), False)
    # parts: strings of two twins at every slice boundary, where the cuts fall; one Mission wholly inside one slice, one that ends
    # in front of the first cut
    body = grid("ascii", 0, 128, 8192) + grid("Cyrillic", 100 * SLICE + 64, 128, 31) + grid("Greek", 64, 128, 40)
    add("parts", ["ascii", "Cyrillic", "Greek", "ascii"], _lay(1 << 20, body), True)
    # ... a dense half and a sparse one: parts of a few findings
    body = grid("ascii", 0, 64, 8192) + grid("Cyrillic", 32, 128, 4096) + grid("ascii", 600 * 1024, 8 * SLICE, 13) + grid("Cyrillic", 600 * 1024 + 32, 24 * SLICE, 4)
    add("small_parts", ["ascii", "Cyrillic"], _lay(1 << 20, body), True)
    return out


def many_missions(n):
    """n > kMergeLists Missions: the four kinds in turn (so Missions 0, 4, 8, 12 and 16 tie at every position, on either side of the
    16th), from the 20th on single-byte encodings with the default filters (they find the ASCII strings too, and more), and the last one
    a Mission with no findings — except for n = kMergeLists + 1, where all have some"""
    base = ["ascii", "Cyrillic", "Greek", "Hebrew"]
    flags = [mission_flag(base[k % 4]) for k in range(min(n, 20))]
    flags += [SINGLE_BYTE[(k - 20) % len(SINGLE_BYTE)] for k in range(20, n)]
    if n != constant("kMergeLists") + 1:
        flags[-1] = mission_flag("Arabic")
    return flags


def many_plant():
    body = grid("ascii", 0, 128, 2048) + grid("Cyrillic", 32, 128, 2048) + grid("Greek", 64, 256, 1024) + grid("Hebrew", 96, 256, 1024)
    return _lay(256 * 1024, body)


COPY_RESIDUES = (0, 1, 15)


def copy_plant(residue):
    """two Missions, 33 000 findings each: one part of more than 1 MiB as 16-byte records, whose strings take `residue` bytes modulo
    16 — the last string is as long as that takes"""
    n = 33000
    placed = sorted(grid("ascii", 0, 32, n) + grid("Cyrillic", 16, 32, n))
    total = sum(len(block_text(kind, i)) for i, (_, kind) in enumerate(placed))
    tail = bytes(LETTERS[(5 * j) % 26].encode()[0] for j in range(4 + (residue - total - 4) % 16))
    data = bytearray(_lay(n * 32 + 64, placed))
    data[n * 32:n * 32 + len(tail)] = tail
    return bytes(data)
