"""Finding::print on the device (stringsext_amd/csrc/sx_print_core.hpp: sx_print_findings_device), compiled as plain host C++ and
driven the way sx_print_dev.hip drives it (tests/native/print_core_host.cpp: the length pass, a scan over the wavefronts' sums, then
wavefront after wavefront the core's three lane loops), against a formatter written here from src/finding.rs:112-155 of the
reference: every combination of the call's parameters, the digit-count edges of the position in all three radices, string lengths
around a 16-byte chunk and a wavefront's range, every misalignment of the output, and a segment whose text straddles the 4 GiB
mark of the text block."""
import ctypes as C
import os
import random
import subprocess

import pytest

import stringsext_amd as sx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "stringsext_amd", "csrc")

POSITIONS = [0, 9, 10, 15, 16, 2 ** 32 - 1, 2 ** 32, 10 ** 19, 2 ** 64 - 1]
LENGTHS = [0, 1, 15, 16, 17, 64, 200]
# (mission_id, label as Finding::print writes it): "ascii" is x-user-defined with print_encoding_as_ascii, src/mission.rs:675-679
ONE = [(0, b"UTF-8")]
SIX = [(0, b"UTF-8"), (1, b"ascii"), (2, b"x-user-defined"), (3, b"x-mac-cyrillic"), (4, b"UTF-16LE"), (5, b"windows-1252")]


def build_print_core():
    """(as tests/native/build_harness.py builds the other cores: g++ on one file, rebuilt when a source is newer)"""
    so, src = os.path.join(NATIVE, "libprint_core_host.so"), os.path.join(NATIVE, "print_core_host.cpp")
    deps = [src, os.path.join(CSRC, "sx_print_core.hpp"), os.path.join(ROOT, "include", "stringsext_amd.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", tmp, src])
        os.replace(tmp, so)
    return so


@pytest.fixture(scope="module")
def core():
    L = C.CDLL(build_print_core())
    L.sxp_print_host.restype = C.c_int
    L.sxp_print_host.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p,
                                 C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.sxp_map.restype, L.sxp_map.argtypes = C.c_void_p, [C.c_uint64]
    L.sxp_unmap.restype, L.sxp_unmap.argtypes = None, [C.c_void_p, C.c_uint64]
    return L


def print_finding(f, n_inputs, radix, no_metadata, missions):
    """Finding::print, src/finding.rs:112-155"""
    out = b"\n"
    if not no_metadata:
        if n_inputs > 1 and f["file_id"] >= 0:
            out += bytes([f["file_id"] + 64]) + b" "                       # 1 -> 'A', 2 -> 'B'
        if radix:
            out += {2: b">", 1: b" ", 0: b"<"}[f["precision"]]               # After, Exact, Before
            out += format(f["position"], {"x": "x", "d": "d", "o": "o"}[radix]).encode()
            out += b"+\t" if f["completes"] else b" \t"
        if len(missions) > 1:
            out += b"(" + bytes([f["mission_id"] + 97]) + b" " + dict(missions)[f["mission_id"]] + b")\t"
    return out + f["s"]


def make_records(rng, specs, missions, file_id):
    """specs: [(position, string length)] -> findings whose strings lie in the arena in another order than the records, with
    gaps between them (the core addresses them by str_off)"""
    recs = []
    for i, (pos, ln) in enumerate(specs):
        recs.append(dict(position=pos, precision=i % 3, completes=(i // 3) % 2, mission_id=missions[i % len(missions)][0],
                         file_id=file_id, s=bytes(rng.randrange(32, 256) for _ in range(min(ln, 300))) * (ln // 300 + 1)))
        recs[-1]["s"] = recs[-1]["s"][:ln]
    order = list(range(len(recs)))
    rng.shuffle(order)
    arena = bytearray(b"\x00" * 3)
    for i in order:
        recs[i]["str_off"] = len(arena)
        arena += recs[i]["s"] + b"\x00" * rng.randrange(0, 3)
    return recs, bytes(arena)


def mission_table(missions):
    tab = bytearray(256 * 16)
    for mid, label in missions:
        assert len(label) <= 14
        tab[mid * 16:mid * 16 + 2 + len(label)] = bytes([1, len(label)]) + label
    return bytes(tab)


def pack(recs, packed):
    arr = ((sx.Finding16 if packed else sx.Finding) * max(1, len(recs)))()
    for i, r in enumerate(recs):
        if packed:
            arr[i] = sx.Finding16(r["position"], r["str_off"], len(r["s"]), r["precision"] | (4 if r["completes"] else 0), r["mission_id"])
        else:
            arr[i] = sx.Finding(r["position"], r["str_off"], len(r["s"]), r["precision"], r["completes"], r["mission_id"], 0, r["file_id"], 0,
                                r["position"] // 4096 & 0xFFFFFFFF)
    return arr


def check(L, recs, arena, packed, missions, n_inputs=1, radix=None, no_metadata=False, misalign=0, file_id=-1):
    want = b"".join(print_finding(r, n_inputs, radix, no_metadata, missions) for r in recs)
    arr = pack(recs, packed)
    abuf = C.create_string_buffer(arena, max(1, len(arena)))
    guard = 64
    raw = C.create_string_buffer(b"\xEE" * (len(want) + 2 * guard + 32), len(want) + 2 * guard + 32)
    text = C.addressof(raw) + guard
    text += (-text) % 16 + misalign
    n = C.c_uint64()
    rc = L.sxp_print_host(C.addressof(arr), len(recs), int(packed), C.addressof(abuf), file_id, n_inputs, ord(radix) if radix else 0,
                          int(no_metadata), len(missions), mission_table(missions), text, 0, C.byref(n))
    assert rc == 0
    assert n.value == len(want)
    got = C.string_at(text, len(want))
    if got != want:
        at = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError(f"text differs at byte {at} of {len(want)}: {got[max(0, at - 40):at + 40]!r} != {want[max(0, at - 40):at + 40]!r}")
    front = text - C.addressof(raw)
    assert C.string_at(C.addressof(raw), front) == b"\xEE" * front, "bytes in front of the text were written"
    assert C.string_at(text + len(want), guard) == b"\xEE" * guard, "bytes behind the text were written"


def edge_specs():
    return [(p, ln) for p in POSITIONS for ln in LENGTHS] + [(12345, 16000), (2 ** 40, 16000), (77, 3)]


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("radix", [None, "x", "d", "o"])
@pytest.mark.parametrize("no_metadata", [False, True])
@pytest.mark.parametrize("n_inputs,file_id", [(1, 3), (2, -1), (2, 3)])
@pytest.mark.parametrize("missions", [ONE, SIX], ids=["one", "six"])
def test_every_parameter_on_the_digit_and_length_edges(core, packed, radix, no_metadata, n_inputs, file_id, missions):
    rng = random.Random(20)
    recs, arena = make_records(rng, edge_specs(), missions, file_id)
    check(core, recs, arena, packed, missions, n_inputs, radix, no_metadata, 0, file_id)


def test_the_formatter_here_writes_what_the_reference_documents():
    f = dict(position=255, precision=1, completes=0, mission_id=1, file_id=2, s=b"hello")
    assert print_finding(f, 2, "x", False, SIX) == b"\nB  ff \t(b ascii)\thello"
    assert print_finding(dict(f, precision=2, completes=1), 1, "o", False, ONE) == b"\n>377+\thello"
    assert print_finding(dict(f, precision=0), 1, "d", True, SIX) == b"\nhello"
    assert print_finding(f, 1, None, False, SIX) == b"\n(b ascii)\thello"


@pytest.mark.parametrize("misalign", range(16))
@pytest.mark.parametrize("count", [1, 63, 64, 65, 4097])
def test_record_counts_and_every_misalignment_of_the_text(core, count, misalign):
    rng = random.Random(count * 16 + misalign)
    specs = [(rng.choice(POSITIONS) if rng.random() < 0.2 else rng.randrange(0, 1 << rng.randrange(1, 64)),
              rng.choice(LENGTHS) if rng.random() < 0.4 else rng.randrange(4, 24)) for _ in range(count)]
    if count >= 64:
        specs[40] = (specs[40][0], 16000)
        specs[63] = (specs[63][0], 16000)   # a wavefront's last line
    packed = (count + misalign) % 2 == 0
    recs, arena = make_records(rng, specs, SIX, 1)
    check(core, recs, arena, packed, SIX, 2, "xdo"[misalign % 3], False, misalign, 1)


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("pad", range(17))
def test_lines_that_end_around_a_chunk_and_a_wavefronts_range(core, packed, pad):
    """64 lines of 16 bytes each fill a wavefront's range exactly; `pad` more bytes in the first string move every line end
    across the chunk boundaries, and the first record of the next wavefront with them"""
    rng = random.Random(pad)
    specs = [(i, 15) for i in range(130)]    # no metadata: '\n' + 15 bytes
    specs[0] = (0, 15 + pad)
    recs, arena = make_records(rng, specs, ONE, -1)
    check(core, recs, arena, packed, ONE, 1, None, True)
    check(core, recs, arena, packed, ONE, 1, "x", False)


@pytest.mark.parametrize("packed", [True, False])
def test_a_segment_whose_text_straddles_the_4_gib_mark(core, packed):
    """the text block is 4 GiB + 1 MiB of untouched anonymous memory; the segment's text begins 2^32 - 5 bytes into it.  Offsets of
    32 bits anywhere between the wavefronts' scan and the stores would put the lines at the block's start."""
    L = core
    size = (1 << 32) + (1 << 20)
    base = (1 << 32) - 5
    rng = random.Random(32)
    recs, arena = make_records(rng, [(rng.randrange(0, 1 << 63), rng.randrange(0, 40)) for _ in range(300)], SIX, 2)
    want = b"".join(print_finding(r, 2, "d", False, SIX) for r in recs)
    block = L.sxp_map(size)
    assert block, "mmap of 4 GiB + 1 MiB of unreserved memory failed"
    try:
        guard = 4096
        C.memset(block + base - guard, 0xEE, guard + len(want) + guard)
        arr, abuf = pack(recs, packed), C.create_string_buffer(arena, len(arena))
        n = C.c_uint64()
        rc = L.sxp_print_host(C.addressof(arr), len(recs), int(packed), C.addressof(abuf), 2, 2, ord("d"), 0, len(SIX), mission_table(SIX),
                              block, base, C.byref(n))
        assert rc == 0 and n.value == len(want)
        assert C.string_at(block + base, len(want)) == want
        assert C.string_at(block + base - guard, guard) == b"\xEE" * guard, "bytes in front of the segment's text were written"
        assert C.string_at(block + base + len(want), guard) == b"\xEE" * guard, "bytes behind the segment's text were written"
        assert C.string_at(block, 8192) == b"\x00" * 8192, "the start of the text block was written: an offset lost its high bits"
    finally:
        L.sxp_unmap(block, size)


def test_a_mission_id_the_context_does_not_have_gets_no_label(core):
    """print_findings (sx_replay.cpp) writes the "(a ...)" part only for a Mission it finds: the core follows"""
    rng = random.Random(5)
    recs, arena = make_records(rng, [(i * 100, 8) for i in range(70)], SIX, -1)
    for r in recs[::7]:
        r["mission_id"] = 9
    arr = pack(recs, True)
    abuf = C.create_string_buffer(arena, len(arena))
    want = b"".join(print_finding(r, 1, "x", False, SIX) if r["mission_id"] != 9 else print_finding(r, 1, "x", False, ONE) for r in recs)
    raw = C.create_string_buffer(len(want) + 64)
    n = C.c_uint64()
    assert core.sxp_print_host(C.addressof(arr), len(recs), 1, C.addressof(abuf), -1, 1, ord("x"), 0, 6, mission_table(SIX),
                               C.addressof(raw), 0, C.byref(n)) == 0
    assert n.value == len(want) and raw.raw[:len(want)] == want
