"""Test helper: planted inputs for stage B's lane-per-region kernels (stringsext_amd/csrc/sx_replay_dev.hip): the fast pre-pass
(replay_fast_region), the copy of the cached outputs (replay_copy_cached_kernel), the stitch (stitch_blocks_kernel,
stitch_chain_kernel), the bounded grid of launch_replay_count, the cut of runs into pieces (split_write_kernel) and the slab cuts.

Every Mission is UTF-8 with every Unicode block let through (characters of one to four bytes are all accepted) and chars_min = 2;
the background is NUL — a valid character that the filter rejects, so it ends a string without ending the decoder call —, a decoder
call is ended by 0xFF, and `E2 82` is a character that the next byte breaks off.  A window is W = 2q bytes of a 4096-byte slice.  A
plant gives every case windows of its own (never a slice's first one, where the reference probes the slice's start), so cases do
not interact, and carries

    data    the bytes
    flags   the Mission, as refconfig.missions(**flags)
    runs    the stretches it planted: (start, end, characters, cut) — cut: the run is cut into pieces at the window starts inside it
    expect  the findings it predicts: (position, precision, string, completes_previous), in the order of the output
    heads   how many entries of the run list (pieces cut) replay a region of their own (replay_heads_kernel)
    fast    how many of those satisfy rules (1)-(5) in front of replay_fast_region — worked out from the numbers planted (where a
            run begins and ends, where its window does, where the call begins), not by decoding bytes
    regions (first byte, is it fast) of every one of the heads
    notes   (position, what) for a failing assertion's message
    extra   what else a plant claims (the stitch plants: which entries of the list are void), by name

The model behind `expect` stands at _Builder.expect.  No random
numbers."""
import os
import re
from collections import namedtuple

SLICE = 4096
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stringsext_amd", "csrc")

Plant = namedtuple("Plant", "data flags runs expect heads fast regions notes extra")


# ---- constants the sizes depend on, from the sources ----

def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(found, what):
    found = set(found)
    assert len(found) == 1, (what, found)
    return found.pop()


def count_grid_cap():
    """-> (workgroups, lanes): the grid of launch_replay_count behind the pre-pass"""
    body = re.search(r"hipError_t launch_replay_count\(.*?\n}\n", _source("sx_replay_dev.hip"), re.S).group(0)
    cap = _one(re.findall(r"P\.hard_list && grid\.x > (\d+)u\) grid\.x = (\d+)u;", body), "grid cap")
    assert cap[0] == cap[1], cap
    lanes = _one(re.findall(r"dim3 grid\(\(unsigned\)\(\(P\.n_runs \+ (\d+)\) / (\d+)\)\);", body), "lanes")
    assert int(lanes[0]) + 1 == int(lanes[1]) and "grid, dim3(%s), lds" % lanes[1] in body, lanes
    return int(cap[0]), int(lanes[1])


def copy_bands():
    """-> [(upper bound of avg_out_bytes or None, G, U)] of launch_replay_write_flagged, in its order"""
    body = re.search(r"hipError_t launch_replay_write_flagged\(.*?\n}\n", _source("sx_replay_dev.hip"), re.S).group(0)
    got = re.findall(r"(?:if|else if) \(avg_out_bytes <= (\d+)\) hipLaunchKernelGGL\(\(replay_copy_cached_kernel<(\d+), (\d+)>\)", body)
    last = re.findall(r"\n\s*else hipLaunchKernelGGL\(\(replay_copy_cached_kernel<(\d+), (\d+)>\)", body)
    assert len(got) == 2 and len(last) == 1, (got, last)
    out = [(int(a), int(g), int(u)) for a, g, u in got] + [(None, int(last[0][0]), int(last[0][1]))]
    assert out[0][0] < out[1][0]
    return out


def avg_out_bytes_rule():
    """the mean launch_replay_write_flagged is given (sx_stage_b.cpp): (findings * sizeof(sx_finding) + string bytes) / standing
    regions; fails if the expression is written otherwise"""
    assert "(nf * sizeof(sx_finding) + nb) / std::max<uint64_t>(1, n_standing), d.stream_b)" in _source("sx_stage_b.cpp")
    return finding_bytes()


def finding_bytes():
    """sizeof(sx_finding), from the binding's mirror of the struct"""
    import ctypes
    import stringsext_amd
    return ctypes.sizeof(stringsext_amd.Finding)


def cache_geom_constants():
    """-> (minimum slot, maximum slot, bytes of a slot per finding) of cache_geom"""
    body = re.search(r"SXD CacheGeom cache_geom\(.*?\n}\n", _source("sx_replay_core.hpp"), re.S).group(0)
    lo = _one(re.findall(r"if \(sb < (\d+)\) sb = (\d+);", body), "minimum slot")
    hi = _one(re.findall(r"if \(sb > (\d+)\) sb = (\d+);", body), "maximum slot")
    per = _one(re.findall(r"g\.cap_f = \(u32\)\(sb / (\d+)\);", body), "per finding")
    assert lo[0] == lo[1] and hi[0] == hi[1] and "n_heads ? arena_bytes / n_heads : %s" % hi[0] in body
    assert "sb &= ~15ull;" in body and "if (g.cap_f < 2) g.cap_f = 2;" in body
    return int(lo[0]), int(hi[0]), int(per)


def cache_geom(arena_bytes, n_heads):
    """-> (slot_bytes, cap_f, cap_b), cache_geom restated"""
    lo, hi, per = cache_geom_constants()
    sb = min(arena_bytes // n_heads if n_heads else hi, hi)
    sb = max(sb, lo) & ~15
    cap_f = max(sb // per, 2)
    return sb, cap_f, sb - cap_f * finding_bytes()


def stitch_block_default():
    """runs per block of the stitch when SX_STITCH_BLOCK is unset, below 2^20 runs"""
    body = re.search(r"inline uint32_t stitch_block_runs\(.*?\n}\n", _source("sx_device.hpp"), re.S).group(0)
    return int(_one(re.findall(r"return n_runs > \(1ull << 20\) \? \d+u : (\d+)u;", body), "stitch block"))


# ---- the window grid, strings ----

def win_start(p, W):
    s = p // SLICE * SLICE
    return s + (p - s) // W * W


def next_win_start(p, W):
    s = p // SLICE * SLICE
    return min(s + (p - s) // W * W + W, s + SLICE)


ONE = "abcdefghijklmnopqrstuvwxyz"
TWO = [chr(0x0410 + k) for k in range(32)]              # Cyrillic capitals
THREE = [chr(c) for c in (0x1E00, 0x0915, 0x1F08, 0x0E01, 0xFB01)]     # leads E1, E0, EF ("All" reads as All-Asian: E2 .. ED are rejected)
FOUR = [chr(c) for c in (0x1F600, 0x1D11E, 0x1F680)]
BAD = 0xFF
TRUNC = b"\xe2\x82"


def _ch(width, k):
    return (None, ONE[k % 26], TWO[k % 32], THREE[k % 5], FOUR[k % 3])[width]


def sized(i, nbytes, first=None):
    """exactly nbytes bytes of characters of 1, 2 and 3 bytes in turn (beginning at another one for every i); first: the width of
    the first character"""
    out, left, j = [], nbytes, 0
    while left:
        w = min(first if first and j == 0 else (1, 2, 3)[(i + j) % 3], left)
        out.append(_ch(w, i + j))
        left -= w
        j += 1
    return "".join(out)


def counted(i, chars, widths=(1, 1, 2, 1, 3, 1, 1)):
    """exactly `chars` characters, of the widths given in turn"""
    return "".join(_ch(widths[j % len(widths)], i + j) for j in range(chars))


def flags_for(q):
    return dict(encodings=["utf-8"], chars_min="2", output_line_len=str(q), unicode_block_filter="All")


# ---- the builder: where runs and call boundaries lie, and what follows from that ----

class _Builder:
    def __init__(self, q, W, pieces=True):
        self.q, self.W, self.pieces = q, W, pieces
        self.d, self.runs, self.bad, self.trunc, self.notes, self.i = bytearray(), [], set(), set(), [], 0
        self.cur = W

    def _room(self, end):
        if len(self.d) < end:
            self.d += bytes(end - len(self.d))

    def take(self, n, what):
        """the next n whole windows of one slice, not its first one and with a whole window behind them; -> the first one's start"""
        W, p = self.W, self.cur
        while True:
            s = p // SLICE * SLICE
            if p == s:
                p += W
            elif (n + 2) * W > SLICE // W * W:
                assert SLICE % W == 0          # more windows than a slice has: they go on through the slices that follow
                break
            elif p + (n + 1) * W > s + SLICE // W * W:
                p = s + SLICE
            else:
                break
        self.cur = p + n * W
        self._room(self.cur + W)
        self.notes.append((p, what))
        return p

    def run(self, rs, s):
        """a run at rs; it must touch nothing that is there"""
        b = s.encode("utf-8")
        self._room(rs + len(b) + 1)
        assert rs > 0 and not any(self.d[rs:rs + len(b)]) and self.d[rs + len(b)] in (0, BAD, TRUNC[0]), (rs, s)
        assert self.d[rs - 1] in (0, 1, BAD) and (rs - 1 not in self.trunc), (rs, s)
        self.d[rs:rs + len(b)] = b
        self.runs.append((rs, rs + len(b), s))
        self.i += 1
        return rs + len(b)

    def malformed(self, pos):
        """0xFF: the decoder call ends in front of it, the next one begins behind it"""
        self._room(pos + 1)
        assert self.d[pos] == 0, pos
        self.d[pos] = BAD
        self.bad.add(pos)

    def broken_off(self, pos):
        """E2 82 and no third byte"""
        self._room(pos + 3)
        assert not any(self.d[pos:pos + 3]), pos
        self.d[pos:pos + 2] = TRUNC
        self.trunc |= {pos, pos + 1}

    def rejected(self, pos, byte=1):
        self._room(pos + 1)
        assert self.d[pos] == 0 and 0 < byte < 0x20
        self.d[pos] = byte

    def plain(self, what):
        """a five-byte run behind a 0xFF in a window of its own: one entry, a region that ends with its window"""
        want = self.take(1, "entry %d: %s" % (len(self.runs), what))
        self.malformed(want + 3)
        self.run(want + 4, sized(self.i, 5))

    def chain(self, k, what, carry=False):
        """k runs 0xFF apart back to back: the first is a head (entry len(runs) now), the others begin in the window where the one
        before ends and are chained; carry: the last one ends with its window.  -> where the last one ends"""
        W = self.W
        want = self.take((k * 12 + 8) // W + 3, "entry %d: %d runs back to back, all but the first chained: %s" % (len(self.runs), k, what))
        at = want + 3
        for j in range(k):
            size = 9
            while any(win_start(p, W) == p for p in (at + 1, at + 1 + size, at + 2 + size)):
                size += 1      # (a run that ends with a window, or a 0xFF there and the next run behind a window start, ends the chain)
            if carry and j == k - 1:
                size = next_win_start(at + 1, W) - (at + 1)
                size += W if size < 3 else 0
            self.malformed(at)
            at = self.run(at + 1, sized(self.i, size))
        return at

    # -- what the numbers planted say

    def _char_starts(self, run):
        rs, _, s = run
        out, p = [], rs
        for c in s:
            out.append(p)
            p += len(c.encode("utf-8"))
        return out

    def entries(self):
        """the run list as stage B gets it: (start, end, continuation, delta, run) with the runs cut into pieces (split_count)"""
        W, out = self.W, []
        for k, run in enumerate(sorted(self.runs)):
            rs, re_, s = run
            starts = [p for p in range(next_win_start(rs, W), re_, 1) if win_start(p, W) == p]
            fe = rs + len(s[0].encode("utf-8")) - 1
            cut = bool(self.pieces and starts and fe < re_ and win_start(fe, W) < rs and (rs - 1) not in self.bad and self.q <= 255)
            edges = [rs] + (starts if cut else []) + [re_]
            for a, b in zip(edges, edges[1:]):
                out.append((a, b, a != rs, a - rs, k))
        return out

    def call_start(self, lo, rs):
        """the start of the decoder call that holds rs, at or behind lo: behind the last 0xFF in [lo, rs)"""
        return max([lo] + [p + 1 for p in self.bad if lo <= p < rs])

    def heads_and_fast(self):
        """-> (heads, fast, [(start, is it fast)] of the heads): rules (1)-(5) of replay_fast_region on the numbers planted"""
        W, q, runs, ent = self.W, self.q, sorted(self.runs), self.entries()
        heads, fast, which = 0, 0, []
        for j, (a, b, cont, delta, k) in enumerate(ent):
            want, wend = win_start(a, W), next_win_start(a, W)
            if j and want < ent[j - 1][1]:
                continue                                            # chained: inside the region of the run before it
            heads += 1
            nxt = ent[j + 1] if j + 1 < len(ent) else None
            starts = self._char_starts(runs[k])
            goes_on = b == wend
            ok = wend <= len(self.d)
            if goes_on:
                ok = ok and nxt is not None and nxt[0] == wend and nxt[2]
            else:
                ok = ok and b + 4 <= wend and (nxt is None or nxt[0] >= wend)
            if cont:
                total = sum(1 for p in starts if p < b)             # characters of the run up to this piece's end
                ok = ok and 0 < delta < 4 * q and total < q
                if not goes_on:
                    before = sum(1 for p, n in zip(starts, starts[1:] + [runs[k][1]]) if n <= a)    # ... that are complete in front of the window
                    ok = ok and before > 0
            else:
                ok = ok and len(starts) < q and self.call_start(want, a) >= want + 4
            fast += ok
            which.append((a, bool(ok)))
        return heads, fast, which

    def expect(self):
        """The findings the reference yields, from where the runs and the 0xFF lie.
        For a run of fewer than q characters: it is yielded by the window in which it is closed — the window that
        holds the byte behind it, or, if only the beginning of a broken-off character lies between it and a window start, the window that
        starts there.  Its position is the start of the decoder call that yields it: behind the last 0xFF in front of the run inside that
        window, or the window start.  The precision is Exact, or Before if a character of the run was complete in front of that window (it was
        carried as leftover; a character across the window start alone is the decoder's business), or After if the call has yielded already.
        A window's text is what was carried plus the characters whose last byte lies in it: while it stays below q characters and the
        run goes on, it is carried; once it has q it is cut every q characters, everything of it is yielded, and from then on every
        window yields its own characters of the run the same way.  All but the run's first finding complete the one before."""
        W, q, out, calls = self.W, self.q, [], set()
        for rs, re_, s in sorted(self.runs):
            starts = self._char_starts((rs, re_, s)) + [re_]
            close = re_
            if re_ in self.trunc:       # only the beginning of a broken-off character between the run and a window start?
                close = next((t for t in (re_ + 1, re_ + 2) if win_start(t, W) == t), re_)
            close = win_start(close, W)
            of = {}                     # a character belongs to the window that holds its last byte
            for j in range(len(s)):
                of.setdefault(win_start(starts[j + 1] - 1, W), []).append(s[j])
            leftover, cut, first = [], False, True
            for at in sorted(set(of) | {close}):
                text = leftover + of.get(at, [])
                if not text or (not cut and len(text) < q and at != close):
                    leftover = text
                    continue
                call = (at, self.call_start(at, rs) if rs >= at else at)
                for c0 in range(0, len(text), q):
                    prec = "After" if call in calls else "Before" if leftover else "Exact"
                    calls.add(call)
                    out.append((call[1], prec, "".join(text[c0:c0 + q]), not first))
                    first = False
                leftover, cut = [], cut or len(text) >= q
        return out

    def plant(self, length=None, **extra):
        if length is not None:
            assert length >= max(r[1] for r in self.runs)
            del self.d[length:]
            self._room(length)
        heads, fast, regions = self.heads_and_fast()
        ent = self.entries()
        cut = {k for _, _, cont, _, k in ent if cont}
        runs = [(rs, re_, len(s), k in cut) for k, (rs, re_, s) in enumerate(sorted(self.runs))]
        return Plant(bytes(self.d), flags_for(self.q), runs, self.expect(), heads, fast, regions, sorted(self.notes), dict(extra, entries=len(ent)))


def describe(plant, pos):
    """the last note at or in front of byte `pos`"""
    best = None
    for p, what in plant.notes:
        if p <= pos:
            best = (p, what)
    return best


def first_difference(plant, got, want):
    """-> None if equal, else the first finding that differs and the case the plant put there"""
    if got == want:
        return None
    k = 0
    while k < len(got) and k < len(want) and got[k] == want[k]:
        k += 1
    g = got[k] if k < len(got) else None
    w = want[k] if k < len(want) else None
    return dict(index=k, got=g, want=w, planted=describe(plant, min(x[0] for x in (g, w) if x)))


# ---- 1. prepass_window ----

PREPASS_GEOMETRY = ((64, 128), (8, 16), (6, 12))
FOLLOWERS = ("nul", "malformed", "broken_off", "run_at_wend-1", "wide_run_at_wend-1", "run_at_wend", "run_at_wend+1")
_plants = {}


def prepass_window(q, W):
    """one case per pair of windows; see the module's text and every case's note"""
    if ("prepass", q) in _plants:
        return _plants["prepass", q]
    b = _Builder(q, W)
    # a six-byte run behind a 0xFF at every offset of the window: the run begins at offsets 1 .. W (the last one: with the next window)
    for o in range(W):
        want = b.take(2, "0xFF at offset %d of the window, a six-byte run behind it" % o)
        b.malformed(want + o)
        b.run(want + o + 1, sized(b.i, 6))
    # 0xFF 0 .. 6 bytes behind the window start, the run 0 .. 2 rejected characters behind it (rule (2): the call starts at want + 4 at least)
    for k in range(7):
        for gap in (0, 1, 2):
            want = b.take(2, "0xFF %d bytes behind the window start, %d NUL, a four-byte run" % (k, gap))
            b.malformed(want + k)
            b.run(want + k + 1 + gap, sized(b.i, 4))
    # ... and no malformed byte at all: the walk back ends at the window start
    for o in (1, 4, 5, 7):
        want = b.take(2, "no 0xFF: a rejected 0x01, then a four-byte run at offset %d" % o)
        b.rejected(want + o - 1)
        b.run(want + o, sized(b.i, 4))
    # where the run ends and what follows it
    for d in range(7):
        for follow in FOLLOWERS:
            n = min(6, W - d - 1)
            at = W + {"run_at_wend-1": -1, "wide_run_at_wend-1": -1, "run_at_wend": 0, "run_at_wend+1": 1}.get(follow, 0)
            if "run" in follow and at <= W - d:
                continue                       # (no room for a NUL between the two)
            want = b.take(2, "a %d-byte run that ends %d bytes in front of the window end, followed by: %s" % (n, d, follow))
            rs = want + W - d - n
            b.malformed(rs - 1)
            re_ = b.run(rs, sized(b.i, n))
            if follow == "malformed":
                b.malformed(re_)
            elif follow == "broken_off":
                b.broken_off(re_)
            elif "run" in follow:              # (wide: its first character lies across the window start, else it ends in front of it)
                b.run(want + at, sized(b.i, 5, first=2 if follow.startswith("wide") else 1))
    # q - 1, q and q + 1 characters (rule (1): fewer than q), bytes and characters differ
    for c in (q - 1, q, q + 1):
        for widths in ((1, 1, 2, 1, 3, 1, 1), (1,)):
            s = counted(b.i, c, widths)
            want = b.take(2 + (len(s.encode()) + 4) // W, "%d characters in %d bytes behind a 0xFF at offset 3" % (c, len(s.encode())))
            b.malformed(want + 3)
            b.run(want + 4, s)
    # every branch of the 16/8/4/1-byte copy tail at every source alignment
    for n in range(4, 41):
        if n + 8 > W and n > 4:
            break
        for a in range(16 if W >= 64 else W - 8 - min(n, W - 8) + 1):
            want = b.take(2, "a run of %d bytes whose first byte is at %d modulo 16" % (n, (4 + a) % 16))
            b.malformed(want + 3 + a)
            b.run(want + 4 + a, sized(b.i, n))
    if SLICE % W:
        # the slice's last window is short (next_win_start clamps): a run in the whole window in front of it, one inside it
        tail = (b.cur // SLICE + 1) * SLICE + SLICE // W * W
        b.cur = tail + SLICE
        b._room(b.cur + W)
        b.notes.append((tail - W, "a four-byte run in the last whole window of a slice, 4 bytes in front of its end"))
        b.malformed(tail - W + 3)
        b.run(tail - W + 4, sized(b.i, 4))
        b.notes.append((tail, "a three-byte run that ends with the slice, in its last window of %d bytes" % (SLICE % W)))
        b.malformed(tail)
        b.run(tail + 1, sized(b.i, SLICE % W - 1))
    # the buffer's last, incomplete window
    want = b.take(2, "a four-byte run in the buffer's last window, which the buffer ends")
    b.malformed(want + 4)
    end = b.run(want + 5, sized(b.i, 4))
    _plants["prepass", q] = b.plant(end + 2)
    return _plants["prepass", q]


# ---- 2. pieces ----

PIECES_GEOMETRY = ((64, 128), (8, 16))


def filled(i, nbytes, width):
    """exactly nbytes bytes: characters of `width` bytes, the last one narrower if need be"""
    out, left, j = [], nbytes, 0
    while left:
        w = min(width, left)
        out.append(_ch(w, i + j))
        left -= w
        j += 1
    return "".join(out)


def pieces(q, W, cut=True, times=1):
    """runs across one, two and three window starts; cut=False: the numbers for SX_NO_PIECES (the same bytes, every run one entry);
    times: all of it that often, for a longer list"""
    if ("pieces", q, cut, times) in _plants:
        return _plants["pieces", q, cut, times]
    b = _Builder(q, W, pieces=cut)
    for _ in range(times):
        deltas = list(range(1, 9)) + [4 * q - 1, 4 * q, 4 * q + 1]
        for crosses in (1, 2, 3):
            for d in deltas:
                for width in (4, 1, 3):    # (4: as few characters as the bytes allow — fewer than q over two window starts —, 1: as many)
                    front = (d + W - 1) // W
                    want = b.take(front + crosses + 1, "a run of %d-byte characters that begins %d bytes in front of a window start and crosses %d" % (width, d, crosses))
                    b.run(want + front * W - d, filled(b.i, d + (crosses - 1) * W + 5, width))
        # a character of two, three and four bytes across the window start, k bytes of it in front; `head` one-byte characters in front of it
        for width in (2, 3, 4):
            for k in range(1, width):
                for head in (0, 1, 3):
                    for crosses in (1, 2):
                        want = b.take(crosses + 2, "a %d-byte character with %d bytes in front of the window start, %d characters before it, the run crosses %d" % (width, k, head, crosses))
                        s = filled(b.i, head, 1) + _ch(width, b.i) + filled(b.i + 1, (crosses - 1) * W + 4, 2)
                        b.run(want + W - k - head, s)
        # q - 1 and q characters up to the end of the piece (rule (4): fewer than q), with one to three of them in front of the window
        for total in (q - 1, q, q + 1):
            for before in (1, 2, 3):
                want = b.take(3, "%d characters in front of the window start, %d up to the run's end" % (before, total))
                b.run(want + W - before, filled(b.i, total, 1))
        # ... and up to the end of a piece that goes on
        for total in (q - 1, q):
            want = b.take(4, "a run whose second piece ends with its window at %d characters" % total)
            m = total - 2                                  # characters whose bytes fill the second window exactly: four-byte ones, one-byte ones and one in between
            x, r = (W - m) // 3, (W - m) % 3
            mid = _ch(1 + r, b.i) if r else ""
            s = filled(b.i, 2, 1) + filled(b.i, 4 * x, 4) + mid + filled(b.i, m - x - (1 if r else 0), 1) + filled(b.i, 5, 1)
            assert len(s.encode()) == 2 + W + 5 and len(s) == total + 5
            b.run(want + W - 2, s)
        # a final piece with a plain run exactly at its window's end; a run that ends exactly there
        for d in (1, 5):
            want = b.take(3, "a run across a window start (%d bytes in front), a plain run exactly at the end of that window" % d)
            b.run(want + W - d, filled(b.i, d + 5, 2))
            b.run(want + 2 * W, sized(b.i, 4))
            want = b.take(3, "a run across a window start (%d bytes in front) that ends with that window" % d)
            b.run(want + W - d, filled(b.i, d + W, 2))
    end = b.cur + W
    _plants["pieces", q, cut, times] = b.plant(end)
    return _plants["pieces", q, cut, times]


# ---- 3. copy_bands ----

def cache_arena_bytes(n_entries, cache_mib=None):
    """the arena of pass 1's cache for a list of n entries (sx_stage_b_plan.hpp cache_arena_bytes, far below the 8 GiB budget), as
    ReplayParams gets it"""
    assert "return std::max<uint64_t>(4096, std::min<uint64_t>(budget, n * 1024));" in _source("sx_stage_b_plan.hpp")
    assert "P.arena_bytes = arena & ~255ull;" in _source("sx_stage_b.cpp")
    budget = (8192 << 20) if cache_mib is None else cache_mib << 20
    return max(4096, min(budget, n_entries * 1024)) & ~255


# per band: q, the lengths of a typical region's strings (the means lie a factor of two inside the band), how many such regions
BAND_SHAPES = ((8, lambda k: [2 + k % 12], 600),
               (64, lambda k: [90 + k % 37, 95 + (k // 3) % 41], 240),
               (100, lambda k: [280 + (k * (j + 1) + 9 * j) % 50 for j in range(6)], 160))


def copy_band(band):
    """The copy of pass 1's cached outputs (replay_copy_cached_kernel<G, U>) is chosen by avg_out_bytes = (findings *
    sizeof(sx_finding) + string bytes) / standing regions of the slab (sx_stage_b.cpp, pass2_and_deliver): band 0, 1, 2 of
    copy_bands().  Every string has a 0xFF in front, so no run is cut into pieces, and the strings of a region follow one another
    in the window where the one before ends: the region is the chain of them.  Typical regions (BAND_SHAPES) set the mean; among
    them lie regions of 1, 2, 3, G/2 and G/2 + 1 short findings, lines of q characters cut from one run, and strings of more than
    4 G bytes; the typical strings' lengths step through every residue modulo 4 against every phase of the destination, strings of
    two bytes included in band 0 (head > nb).  extra: band (lower, upper bound), G, mean (the plant's own), findings (per special region)"""
    if ("band", band) in _plants:
        return _plants["band", band]
    bands = copy_bands()
    upper, G, _ = bands[band]
    lower = bands[band - 1][0] if band else 0
    q, shape, n_typical = BAND_SHAPES[band]
    W = 2 * q
    b = _Builder(q, W)
    special = {}

    def region(lengths, what, width=None):
        need = sum(n + 1 for n in lengths) + 4
        want = b.take((need + W - 1) // W + 1, what)
        at = want + 3
        for n in lengths:
            if win_start(at + 1, W) == at + 1:        # (a run that begins with a window is a region of its own)
                at += 1
            b.malformed(at)
            # (fewer than q characters, or the next string would complete a cut line; two at least)
            at = b.run(at + 1, filled(b.i, n, width or (4 if n >= q else 1 if n < 4 else 1 + b.i % 3)))
        return want
    specials = [(k, [3 + (k + j) % 5 for j in range(k)], "%d short findings in one region" % k) for k in (1, 2, 3, G // 2, G // 2 + 1)]
    specials.append((None, [4 * G + 1 + band], "a string of more than 4 G bytes"))
    specials.append((None, [4 * G + 7], "a string of more than 4 G bytes"))
    specials.append((None, [3 * q + 2], "lines of q characters cut from one run of one-byte characters"))
    every = n_typical // (len(specials) + 1)
    for k in range(n_typical):
        if k % every == 1 and specials:
            nf, lengths, what = specials.pop(0)
            pos = region(lengths, what, width=1 if "lines" in what else None)
            if nf:
                special[pos] = nf
        region(shape(k), "a typical region: strings of %s bytes" % shape(k))
    assert not specials
    nf, nb = len(b.expect()), sum(len(f[2].encode("utf-8")) for f in b.expect())
    heads = b.heads_and_fast()[0]
    mean = (nf * avg_out_bytes_rule() + nb) // heads
    _plants["band", band] = b.plant(b.cur + W, band=(lower, upper), G=G, mean=mean, findings=special)
    return _plants["band", band]


def cache_edge():
    """SX_REPLAY_CACHE_MIB=0: the arena is 4096 bytes, so with more than 25 heads cache_geom gives the minimum slot of 160 bytes
    — 2 findings, 96 bytes — to the first 25 of them and none to the others.  Regions whose output is exactly 2 findings, exactly
    96 bytes, both, and one more of either (no pad: replay_write_flagged_kernel replays them a second time) come first.
    extra: slot = (slot_bytes, cap_f, cap_b), slots = how many heads get one, regions = [(findings, bytes)] of the heads, fast = the
    regions the pre-pass takes with these slots"""
    if "cache_edge" in _plants:
        return _plants["cache_edge"]
    q, W = 64, 128
    b = _Builder(q, W)
    arena = cache_arena_bytes(64, cache_mib=0)
    slot, cap_f, cap_b = cache_geom(arena, 64)
    shapes = [[4], [5, 6], [5, 6, 7], [cap_b], [cap_b + 1], [cap_b // 2, cap_b - cap_b // 2], [cap_b // 2, cap_b - cap_b // 2 + 1],
              [cap_b - 3], [3, 4, 5], [cap_b - 3, 3]] + [[4 + k % 7] for k in range(50)]
    regions = []
    for lengths in shapes:
        need = sum(n + 1 for n in lengths) + 4
        want = b.take((need + W - 1) // W + 1, "a region of %d findings, %d bytes (a slot holds %d, %d)" % (len(lengths), sum(lengths), cap_f, cap_b))
        at = want + 3
        for n in lengths:
            if win_start(at + 1, W) == at + 1:
                at += 1
            b.malformed(at)
            at = b.run(at + 1, filled(b.i, n, 2))
        regions.append((len(lengths), sum(lengths)))
    # the pre-pass takes a region only if it has a slot and its string fits there (replay_fast_kernel: room, nb <= cap_b)
    size = {rs: re_ - rs for rs, re_, _ in b.runs}
    fast = sum(1 for k, (a, ok) in enumerate(b.heads_and_fast()[2]) if ok and k < arena // slot and size[a] <= cap_b)
    _plants["cache_edge"] = b.plant(b.cur + W, slot=(slot, cap_f, cap_b), slots=arena // slot, regions=regions, fast=fast)
    return _plants["cache_edge"]


# ---- 4. stitch ----

STITCH_BLOCKS = (7, 64, None)          # SX_STITCH_BLOCK; None: unset, stitch_block_default()
STITCH_CHUNK = 16 * SLICE


def stitch(block):
    """A list whose entry k is planted for blocks of S = `block` runs (None: the default), so that the void regions lie where
    stitch_blocks_kernel and stitch_chain_kernel have their edges.  The units, all UTF-8 (a splittable Mission does overrun: a run
    of fewer than q characters that ends with its window is carried as leftover, so its region goes on into the next window, and a
    run that begins there is no chained run — its window does not start in front of that end — but a head, which is void):
        plain    one run in a window of its own
        pair     a run that ends with its window, a run in the next window: the second is void
        stairs   a run that ends with its window, then k runs that each begin in the next window and end with it: all k are void
        chain    k runs 0xFF apart back to back: the first is a head, the others are chained (no region of their own)
    extra: S; void = {what: index in the list}; chained = {what: index}; n = entries"""
    S = block or stitch_block_default()
    if ("stitch", S) in _plants:
        return _plants["stitch", S]
    q, W = 64, 128
    b = _Builder(q, W)
    void, chained = {}, {}

    def n():
        return len(b.runs)

    def plain(upto):
        while n() < upto:
            b.plain("a plain run")

    def stairs(k, what, name):
        """the overrunning run is entry n(), the void ones n() + 1 .. n() + k"""
        want = b.take(k + 2, "entry %d: a run that ends with its window, then %d void run(s): %s" % (n(), k, what))
        b.malformed(want + W - 7)
        b.run(want + W - 6, sized(b.i, 6))
        for j in range(k):
            if j == k - 1:
                void[name] = n()
                b.run(want + (j + 1) * W + 2, sized(b.i, 4))
            else:
                b.run(want + (j + 1) * W + 2, sized(b.i, W - 2))

    def chain(k, what, name, carry=False):
        end = b.chain(k, what, carry)
        chained[name] = n() - 1
        return end

    def at_block(blk, index):
        plain(blk * S + index)
        assert n() == blk * S + index, (n(), blk, index, S)

    lane = lambda x: min(x, S - 1)
    # block 1: its first run is void (the run in front of it is the last of block 0): the chain kernel's repair meets the block's own chain again
    at_block(1, -1)
    stairs(1, "the first run of block 1", "first of a block")
    # block 2: two void runs inside one group of 64 (one round each), one at its last lane
    at_block(2, 2)
    stairs(1, "lane 3 of block 2", "lane 3")
    at_block(2, lane(20) - 1)
    stairs(1, "a second one in the same group", "second in a group")
    if S >= 64:
        at_block(2, 62)
        stairs(1, "lane 63 of the group", "lane 63")
    if S > 64:
        at_block(3, 63)
        stairs(1, "lane 0 of the block's second group (E carried from the group before)", "lane 0 of a second group")
        at_block(3, 70)
        stairs(2, "two void runs in a row in the second group", "two in a row")
    # block 5 begins with chained runs: its first candidate is not its first run
    at_block(5, -2)
    chain(5, "the head lies in block 4, block 5 begins with chained runs", "block begins chained")
    # blocks 7 and 8: the last run of block 6 overruns all of block 7 (the repair runs to the block's end) and the first two runs of block 8
    at_block(7, -1)
    stairs(S + 2, "all of block 7 and two runs of block 8", "two blocks overrun")
    # block 10 holds chained runs only; the chain's last run ends with its window, the first run of block 11 is void
    at_block(10, -1)
    end = chain(S + 1, "all of block 10, no region of its own between the overrunning block and its victim", "a whole block chained", carry=True)
    assert n() == 11 * S and win_start(end, W) == end
    b.cur = max(b.cur, end + W)
    b._room(b.cur + W)
    b.notes.append((end, "entry %d: the run behind a chain that ends with its window: void" % n()))
    void["behind a chained block"] = n()
    b.run(end + 2, sized(b.i, 4))
    # behind 64 and 128 blocks: the summaries stitch_chain_kernel fetches while it chains the 64 before
    for blk in (64, 65, 128, 129) if S == 7 else (64, 65):
        at_block(blk, -1)
        stairs(1, "the first run of block %d" % blk, "first of block %d" % blk)
    plain(n() + 3)
    # the first window of a chunk of STITCH_CHUNK bytes holds a run that ends with it, the second window a run: the host replays the
    # chunk's first region from the carried state, and where it ends (E0) is behind the first head of the chunk's list
    if block == 7:
        c = (b.cur + STITCH_CHUNK) // STITCH_CHUNK * STITCH_CHUNK
        b.cur = c + 2 * W
        b._room(b.cur + W)
        b.notes.append((c, "entry %d: a chunk's first window holds a run that ends with it; the run in the second window is void (E0)" % n()))
        b.malformed(c + W - 7)
        b.run(c + W - 6, sized(b.i, 6, first=1))
        void["overrun by the entry region"] = n()
        b.run(c + W + 2, sized(b.i, 4))
        plain(n() + 2 * S)
    _plants["stitch", S] = b.plant(b.cur + W, S=S, void=void, chained=chained, n=n())
    return _plants["stitch", S]


# ---- 5. count_trips ----

TRIPS_GEOMETRY = (8, 16)


def count_trips(one_more):
    """one region per pair of windows that the pre-pass must refuse — a rejected 0x01 and no malformed byte in front of a three-letter
    run, so its call starts with the window (rule (2)) —: as many as one trip of replay_count_cached_kernel's bounded grid visits
    behind the pre-pass (count_grid_cap()), and (one_more) one more, which a lane visits on a second trip.  Nothing in the buffer's
    first pair of windows (the host's entry region)"""
    q, W = TRIPS_GEOMETRY
    wgs, lanes = count_grid_cap()
    n = wgs * lanes + (1 if one_more else 0)
    cell = bytearray(2 * W)
    cell[0] = 1
    data = bytes(2 * W) + b"".join(bytes(cell[:1]) + bytes((97 + (k + j) % 26) for j in range(3)) + bytes(2 * W - 4) for k in range(n))
    expect = [((k + 1) * 2 * W, "Exact", "".join(chr(97 + (k + j) % 26) for j in range(3)), False) for k in range(n)]
    runs = [((k + 1) * 2 * W + 1, (k + 1) * 2 * W + 4, 3, False) for k in range(n)]
    notes = [(2 * W, "%d regions of one three-letter run behind a 0x01 at its window's start" % n)]
    return Plant(data, flags_for(q), runs, expect, n, 0, None, notes, dict(trip=wgs * lanes))


# ---- 6. slabs ----

SLABS = (2, 5, 64)
SLAB_CHAIN_SHAPES = {"small": (40, 60, 12), "large": (300, 340, 40)}      # plain runs, a chain, plain runs behind it


def slab_min_entries(slabs):
    """the entries a list needs to be replayed in `slabs` slabs with SX_SLABS (sx_stage_b.cpp slabs_wanted; with fewer: one slab)"""
    factor = _one(re.findall(r"if \(ctx->sw\.slabs\) \{ K = \(size_t\)ctx->sw\.slabs; if \(!can \|\| n < (\d+) \* K\) K = 1; \}", _source("sx_stage_b.cpp")), "slabs")
    return int(factor) * slabs


def slab_chains(tail, shape="small"):
    """a list of plain runs, then a chain of more than as many chained runs; tail: and plain runs behind it, fewer than a fifth.
    slab_cuts_kernel's cuts from half of the list on fall on chained runs and walk — tail: to the first run behind the chain; else
    to the list's end (i == n_runs).  extra: entries, chain = (first, last) chained entry"""
    if ("slab_chains", tail, shape) in _plants:
        return _plants["slab_chains", tail, shape]
    n_plain, k, n_tail = SLAB_CHAIN_SHAPES[shape]
    b = _Builder(64, 128)
    for _ in range(n_plain):
        b.plain("a plain run")
    first = len(b.runs) + 1
    b.chain(k, "more than half of the list")
    last = len(b.runs) - 1
    for _ in range(n_tail if tail else 0):
        b.plain("a plain run behind the chain")
    _plants["slab_chains", tail, shape] = b.plant(b.cur + b.W, chain=(first, last))
    return _plants["slab_chains", tail, shape]


def slab_plants(slabs):
    """the plants replayed with SX_SLABS=slabs: the pieces plants and the chains, of those shapes that have entries enough for it"""
    out = [pieces(q, W, times=t) for q, W in PIECES_GEOMETRY for t in (1, 2)] + [slab_chains(tail, shape) for shape in sorted(SLAB_CHAIN_SHAPES) for tail in (False, True)]
    out = [p for p in out if p.extra["entries"] >= slab_min_entries(slabs)]
    assert len(out) >= 2 and any("chain" in p.extra for p in out), slabs
    return out
