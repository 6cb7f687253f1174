"""Planted buffers for the slabs of a busy Mission next to quiet ones (tests/test_slab_plant.py on the CPU, tests/test_gpu_slabs_multi.py
on the device): `-e utf-8 -e utf-16le -e utf-16be -u African`, a background no Mission reads a character in, and on it

 * one short UTF-8 stretch every 512 bytes, inside one 128-byte window (a run of its own, a region of its own), a few thousand in all;
 * a few UTF-16 strings per block, little and big endian.

The buffer is BLOCKS (12) equal blocks, so the UTF-8 Mission's run list is 12 equal parts whatever stage A makes of a run (it cuts a
long one into a piece per window): a list cut into 2, 3 or 4 slabs (csrc/sx_replay_dev.hip slab_cuts_kernel: at the first run at or
behind n / K * j that starts a region) is cut at the first run of a block.  Two flavours say what lies there:

 "u16"   the block begins with a UTF-16LE string at its byte 0, a UTF-16BE string 18 bytes in and its first UTF-8 stretch 40 bytes
         in, and ends with a UTF-16BE string 20 bytes in front of the next block: findings of the other Missions a few bytes on
         either side of the cut and one exactly at it.
 "long"  a UTF-8 stretch of 300 bytes begins 20 bytes in front of every block start: the run is open across the cut (and across the
         boundary of two scan calls or two pieces that end on a block), its region begins in the window in front of it.
"""
import random

BLOCKS = 12
BLOCK = 512 * 1024
STEP = 512
N = 6                       # -n: characters a finding needs
FLAGS = dict(encodings=["utf-8", "utf-16le", "utf-16be"], chars_min=str(N), unicode_block_filter="African")
WORDS = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789/._-"
WIDE = "אבגדהוזחטיכלמנסעפצקרשת"   # Hebrew: two bytes in UTF-8, inside -u African


def quiet(rng, n):
    """bytes no Mission reads a character in: lone UTF-8 continuation bytes; as UTF-16 units U+8080..U+BFBF"""
    return bytearray(rng.choices(range(0x80, 0xC0), k=n))


def word(rng, lo, hi, wide=True):
    n = rng.randrange(lo, hi + 1)
    alphabet = WORDS + (WIDE if wide else "")
    return "".join(rng.choice(alphabet) for _ in range(n))


class Plant:
    def __init__(self, flavour, data, utf8, utf16le, utf16be):
        self.flavour, self.data = flavour, data
        self.utf8, self.utf16le, self.utf16be = utf8, utf16le, utf16be   # [(start, end, chars)] as the oracle's runs report them


_cache = {}


def plant(flavour, blocks=BLOCKS):
    key = (flavour, blocks)
    if key in _cache:
        return _cache[key]
    assert flavour in ("u16", "long")
    rng = random.Random(0x51AB5 + (flavour == "long"))
    total = blocks * BLOCK
    data = quiet(rng, total)
    utf8, le, be = [], [], []

    def put8(at, text):
        raw = text.encode()
        data[at:at + len(raw)] = raw
        utf8.append((at, at + len(raw), len(text)))

    def put16(at, text, big):
        assert at % 2 == 0
        raw = text.encode("utf-16-be" if big else "utf-16-le")
        data[at:at + len(raw)] = raw
        (be if big else le).append((at, at + len(raw), len(text)))

    # one block, repeated: the same lengths in every block (the run list must be `blocks` equal parts), other letters
    shape = random.Random(7)
    lens = [shape.randrange(N, 21) for _ in range(BLOCK // STEP)]
    for b in range(blocks):
        base = b * BLOCK
        for i, n in enumerate(lens):
            at = base + i * STEP + 40
            if flavour == "long" and i == 0:
                continue                                    # (the long stretch lies here)
            # 40 + 2 * 20 bytes at most: inside the window that begins at base + i * STEP
            put8(at, "".join(rng.choice(WORDS + WIDE) for _ in range(n)))
        if flavour == "u16":
            put16(base, word(rng, N, 8, wide=False), big=False)             # exactly at the block start: 16 bytes at most
            put16(base + 18, word(rng, N, 8, wide=True), big=True)          # a few bytes behind it, ends in front of byte 40
            put16(base + BLOCK - 20, word(rng, N, 8, wide=True), big=True)  # ... and in front of the next one (ends 4 bytes before it)
        else:
            start = base - 20 if b else 0
            put8(start, "".join(rng.choice(WORDS) for _ in range(base + 280 - start)))   # ASCII: a byte a character
            if b == blocks - 1:
                put8(total - 20, "".join(rng.choice(WORDS) for _ in range(20)))          # (the last block ends as the others do)
        # the other Missions' findings inside the block, between two UTF-8 stretches
        put16(base + 100 * STEP + 200, word(rng, N, 30, wide=True), big=False)
        put16(base + 700 * STEP + 330, word(rng, N, 30, wide=True), big=True)
    utf8.sort(); le.sort(); be.sort()
    _cache[key] = Plant(flavour, bytes(data), utf8, le, be)
    return _cache[key]
