"""Test helper: planted inputs for the fused scan (stringsext_amd/csrc/sx_fused.hip).

The kernel's header argues that no stretch of accepted units is lost at a 1 KiB tile edge: a qualifying stretch has an aligned group of
high bytes in some tile, that tile is classified, an open carry forces the next one, a skipped tile's carry word is recomputed or known
to be 0 — from any of the fast loop's three trip positions.  An ATLAS turns that argument into data: one stretch per EVENT, an event
being one combination of

  encoding    UTF-16LE, UTF-16BE (`a..z`), UTF-8 (ASCII and a two-byte character alternating, beginning with either)
  length      n-1, n, n+1, n+6, 2n+1 characters around the threshold n
  offset      of the stretch's first byte relative to a tile edge: every value from -(2(2n+1)+4) to +5 — the stretch ends in front
              of the edge, on it, behind it, begins up to 12 and more bytes in front of it, straddles it with its only aligned
              group on either side, at both byte phases
  background  what lies around it: bytes whose tiles every UTF-16 prefilter skips and whose last byte cannot be good (FF), skipped
              tiles whose last unit's high byte passes the mask for one byte order only (FF 00 FF FF, laid at every phase of the
              tile grid), and bytes whose high bytes all pass while no unit is accepted (no tile is skipped)

Each event is planted kCopies = 3 times, kSpacing = 5 (UTF-8: 7) tiles apart: the events cannot touch, and as that is no multiple of
3 the three copies have their edge tile at the three values of (tile index mod 3), i.e. at the fast loop's three trip positions.  Everything is
deterministic: no random numbers."""
from collections import namedtuple

TILE = 1024
kSpacing = 5     # tiles from one event's edge to the next one's (UTF-16: a Mission sees a stretch at one stream parity only)
kSpacing8 = 7    # ... in a UTF-8 atlas, where every stretch is a run at either parity
kLead = 2        # the edge lies this many tiles into the event's own stretch of background
kCopies = 3
LETTERS = "abcdefghijklmnopqrstuvwxyz"
TWO_BYTE = "Ж"   # U+0416: inside -u Cyrillic

# backgrounds: skipped / skipped with a last unit that may pass / never skipped.  No unit that any phase of these patterns forms, or that
# one of their bytes forms with a stretch's 00, is accepted by a filter of ASCII and one range above U+0100 (-u African, Cyrillic,
# Greek, None): 00FF, FF00, FFFF, 0001, 0100
BACKGROUNDS = (b"\xff", b"\xff\x00\xff\xff", b"\x00\x01")

UTF16 = ("utf-16le", "utf-16be")
UTF8 = ("utf-8:a", "utf-8:b")    # ASCII first / the two-byte character first

Event = namedtuple("Event", "enc chars off bg copy edge_tile start end")
Atlas = namedtuple("Atlas", "data planted events n spacing")


def lengths(n):
    return (n - 1, n, n + 1, n + 6, 2 * n + 1)


def offsets(n):
    return range(-(2 * (2 * n + 1) + 4), 6)


def stretch(enc, chars):
    if enc == "utf-16le" or enc == "utf-16be":
        return "".join(LETTERS[i % 26] for i in range(chars)).encode("utf-16-le" if enc == "utf-16le" else "utf-16-be")
    first = 0 if enc == "utf-8:a" else 1
    return "".join(LETTERS[i % 26] if (i + first) % 2 == 0 else TWO_BYTE for i in range(chars)).encode("utf-8")


def background(pattern, phase, size):
    """`size` bytes of `pattern` repeated, beginning at its byte `phase`"""
    ph = phase % len(pattern)
    return (pattern * (size // len(pattern) + 2))[ph:ph + size]


def build(n, encodings, backgrounds=BACKGROUNDS, spacing=kSpacing):
    """-> Atlas(data, planted, events, n): planted[i] = (start, end, chars) of events[i]'s stretch, in input order"""
    kinds = [(enc, chars, off, bg) for bg in range(len(backgrounds)) for off in offsets(n) for chars in lengths(n) for enc in encodings]
    n_events = len(kinds) * kCopies
    data = bytearray()
    events = []
    for e in range(n_events):
        enc, chars, off, bg = kinds[e // kCopies]
        data += background(backgrounds[bg], e, spacing * TILE)    # (the pattern's phase against the tile grid changes from event to event)
        edge_tile = e * spacing + kLead
        s = stretch(enc, chars)
        start = edge_tile * TILE + off
        data[start:start + len(s)] = s
        events.append(Event(enc, chars, off, bg, e % kCopies, edge_tile, start, start + len(s)))
    data += background(backgrounds[0], 0, kLead * TILE)
    return Atlas(bytes(data), [(ev.start, ev.end, ev.chars) for ev in events], events, n, spacing)


# ---- the atlases and Mission sets the tests use: (kind, n, filter) -> build() ----

SETS = {
    "c3": ["utf-8", "utf-16le", "utf-16be"],       # the headline's three Missions: one launch
    "u8_le": ["utf-8", "utf-16le"], "u8_be": ["utf-8", "utf-16be"], "le_be": ["utf-16le", "utf-16be"],
    "u8": ["utf-8"],                               # the UTF-8 range Mission alone
}
SET_MASK = {"c3": 0b111, "u8_le": 0b11, "u8_be": 0b11, "le_be": 0b11, "u8": 0b1}

# (Mission set, atlas): UTF-16 thresholds 2 | 3 (no prefilter | pairs), 6 | 7 (pairs | groups of four; candidate test of 12 | 14
# bytes) and 10; UTF-8 thresholds 11 .. 15 (candidate test below, at and above 12 bytes); -u Greek (U+0380..U+03FF) and -u None (ASCII only): prefilter masks 3 and 0 instead of 7
ATLAS_CASES = (
    [(s, ("u16", n, "African")) for n in (2, 3, 6, 7, 10) for s in ("c3", "u8_le", "u8_be", "le_be")]
    + [(s, ("u16", n, flt)) for n, flt in ((3, "Greek"), (7, "Greek"), (3, "None"), (7, "None")) for s in ("c3", "le_be")]
    + [(s, ("u8", n, "Cyrillic")) for n in (11, 12, 13, 14, 15) for s in ("c3", "u8")]
    + [("u8_le", ("u8", 12, "Cyrillic")), ("u8_be", ("u8", 13, "Cyrillic"))]
)
# thresholds that differ within one launch: the host picks the weakest prefilter (pairs for 7 with 4, none for 10 with 2)
MIXED_CASES = [((7, 4), 2), ((4, 7), 2), ((10, 2), 0), ((2, 10), 0)]

_cache = {}


def atlas(key):
    """the atlas of `key` = (kind, n, filter), built once (the last two are kept)"""
    if key not in _cache:
        while len(_cache) >= 2:
            _cache.pop(next(iter(_cache)))
        kind, n, flt = key
        _cache[key] = build(n, UTF16) if kind == "u16" else build(n, UTF8, spacing=kSpacing8)
    return _cache[key]


def set_flags(set_name, key):
    return dict(encodings=SETS[set_name], chars_min=str(key[1]), unicode_block_filter=key[2])


def mixed_flags(le, be):
    return dict(encodings=[f"utf-16le,{le}", f"utf-16be,{be}"], unicode_block_filter="African")


def mission_name(enc):
    return enc.split(":")[0]


def expected(atlas, encoding, n, parity):
    """The planted stretches a Mission of `encoding` ("utf-8", "utf-16le", "utf-16be") with threshold n reports at this stream parity"""
    if encoding == "utf-8":
        return [(ev.start, ev.end, ev.chars) for ev in atlas.events if mission_name(ev.enc) == encoding and ev.chars >= n]
    out = []
    for ev in atlas.events:
        if ev.enc not in UTF16:
            continue
        if ev.enc == encoding:
            run = (ev.start, ev.end, ev.chars) if (ev.start - parity) % 2 == 0 else None    # (at the other phase: `a` as a high byte)
        elif (ev.start - parity) % 2 == 0:
            run = None
        elif encoding == "utf-16le":
            # 00 a 00 b 00 c | x read one byte on as (a 00)(b 00)(c x): the last unit counts if the background goes on with 00
            k = ev.chars if atlas.data[ev.end] == 0 else ev.chars - 1
            run = (ev.start + 1, ev.start + 1 + 2 * k, k)
        else:
            # x | a 00 b 00 c 00 read one byte earlier as (x a)(00 b)(00 c): the first unit counts if the background ended with 00
            k = ev.chars if atlas.data[ev.start - 1] == 0 else ev.chars - 1
            run = (ev.end - 1 - 2 * k, ev.end - 1, k)
        if run and run[2] >= n:
            out.append(run)
    return out


def describe(atlas, pos):
    """the event whose ground holds byte `pos` (for a failing assertion's message)"""
    e = min(max(pos // (atlas.spacing * TILE), 0), len(atlas.events) - 1)
    return atlas.events[e]


def first_difference(atlas, got, want):
    """-> None if equal, else a description of the first run that differs and of the event it belongs to"""
    if got == want:
        return None
    k = 0
    while k < len(got) and k < len(want) and got[k] == want[k]:
        k += 1
    g = got[k] if k < len(got) else None
    w = want[k] if k < len(want) else None
    ev = describe(atlas, (w or g)[0])
    return dict(index=k, got=g, want=w, event=ev._asdict(), edge_tile_mod3=ev.edge_tile % 3)


# ---- the end of the input ----

END_RESIDUES = (0, 1, 2, 15, 16, 17, 31, 32, 33, 1023)


def end_buffers(residue, n):
    """Buffers of 1 to 5 tiles whose length is `residue` modulo 1 KiB, each with one stretch at its very end: it ends at the last byte,
    one byte before it, or (UTF-16) with half a unit left over.  -> [(label, data)]"""
    out = []
    for tiles in range(1, 6):
        size = (tiles - 1) * TILE + (residue if residue else TILE)
        for bi, bg in enumerate((b"\xff", b"\x00\x01")):
            for enc in UTF16 + UTF8[:1]:
                for how in ("last", "before", "dangling"):
                    if how == "dangling" and enc not in UTF16:
                        continue
                    chars = n if (tiles + bi) % 2 else 3 * n + 1
                    s = stretch(enc, chars)
                    if how == "before": s += bg[:1]
                    if how == "dangling": s += stretch(enc, chars + 1)[len(s):len(s) + 1]   # the first byte of one more unit
                    if len(s) > size:
                        s = s[len(s) - size:]
                    data = bytearray(background(bg, 0, size))
                    data[size - len(s):] = s
                    out.append((f"{tiles}t+{residue}/{bi}/{enc}/{how}", bytes(data)))
    return out


# ---- a skipped tile in front of the fast loop's first trip ----

def first_trip_buffers(n, top=None):
    """Eight tiles of FF.  Tile 0 opens the input, so nothing forces its classification: it is skipped when it holds no aligned group.
    The stretch begins in it and has its group in tile 1, the first tile the fast loop handles — with no register set that still
    holds the tile in front.  top: every other character is this code point — the highest the filter accepts, whose high byte has
    every bit of the prefilter's mask — instead of a letter.  -> [(label, data)]"""
    out = []
    for enc in UTF16:
        for chars in (n, n + 1, n + 6, 2 * n + 1):
            for off in range(-2 * chars + 1, 0):
                data = bytearray(b"\xff" * (8 * TILE))
                s = stretch(enc, chars)
                if top is not None:
                    text = "".join(chr(top) if i % 2 else LETTERS[i % 26] for i in range(chars))
                    s = text.encode("utf-16-le" if enc == "utf-16le" else "utf-16-be")
                data[TILE + off:TILE + off + len(s)] = s
                out.append((f"{enc}/{chars}/{off}", bytes(data)))
    return out
