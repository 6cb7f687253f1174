"""The substring selection over a device-resident result (stringsext_amd/csrc/sx_select_core.hpp: sx_result_select_device), compiled
as plain host C++ and driven the way sx_select_dev.hip drives it (tests/native/select_core_host.cpp: wavefront after wavefront the
load step, the vote, the scan of the range or the walk, the ballot; a scan over the counts; the placement; the ordered gather of
sx_result_core.hpp), against Python's `p in s` — bytes.lower() folds 'A'..'Z' and nothing else, as SX_SELECT_ASCII_NOCASE does.
The source arena ends where a page without access begins: the core may read nothing behind the last string."""
import ctypes as C
import os
import random
import subprocess

import pytest

import stringsext_amd as sx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "stringsext_amd", "csrc")
NOCASE, INVERT = sx.SX_SELECT_ASCII_NOCASE, sx.SX_SELECT_INVERT


def build_select_core():
    """(as tests/native/build_harness.py builds the other cores: g++ on one file, rebuilt when a source is newer)"""
    so, src = os.path.join(NATIVE, "libselect_core_host.so"), os.path.join(NATIVE, "select_core_host.cpp")
    deps = [src, os.path.join(NATIVE, "guarded_host.hpp"), os.path.join(NATIVE, "select_pass2_host.hpp"), os.path.join(CSRC, "sx_select_core.hpp"), os.path.join(CSRC, "sx_result_core.hpp"), os.path.join(ROOT, "include", "stringsext_amd.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", tmp, src])
        os.replace(tmp, so)
    return so


@pytest.fixture(scope="module")
def core():
    L = C.CDLL(build_select_core())
    u64p = C.POINTER(C.c_uint64)
    L.sxs_select_host.restype = C.c_int
    L.sxs_select_host.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_char_p, C.POINTER(C.c_uint32), C.c_int, C.c_uint32,
                                  C.c_void_p, C.c_void_p, C.c_uint64, u64p, u64p, u64p, u64p]
    L.sxs_guarded.restype, L.sxs_guarded.argtypes = C.c_void_p, [C.c_uint64, C.POINTER(C.c_void_p), u64p]
    L.sxs_unmap.restype, L.sxs_unmap.argtypes = None, [C.c_void_p, C.c_uint64]
    return L


def matches(s, patterns, nocase):
    """the rule of include/stringsext_amd.h, with Python's substring search"""
    if nocase:
        s, patterns = s.lower(), [p.lower() for p in patterns]
    return any(p in s for p in patterns)


def lay_out(strings, layout, rng):
    """(str_off per string, arena): "packed" = back to back in record order, as every merged segment; "scattered" = any order, gaps"""
    if layout == "packed":
        offs, at = [], 0
        for s in strings:
            offs.append(at); at += len(s)
        return offs, b"".join(strings)
    order = list(range(len(strings)))
    rng.shuffle(order)
    offs, arena = [0] * len(strings), bytearray(b"\x00" * rng.randrange(0, 4))
    for i in order:
        offs[i] = len(arena)
        arena += strings[i] + b"\x00" * rng.randrange(0, 3)
    return offs, bytes(arena)


def records(strings, offs, packed):
    arr = ((sx.Finding16 if packed else sx.Finding) * max(1, len(strings)))()
    for i, s in enumerate(strings):
        if packed:
            arr[i] = sx.Finding16(1000 + 7 * i, offs[i], len(s), i % 7, i % 5)
        else:
            arr[i] = sx.Finding(1000 + 7 * i, offs[i], len(s), i % 3, (i // 3) % 2, i % 5, 0, 3, 0, (1000 + 7 * i) // 4096)
    return arr


def fields(r, packed):
    return (r.position, r.str_len, r.flags, r.mission_id) if packed else \
        (r.position, r.str_len, r.precision, r.completes_previous, r.mission_id, r.input_file_id, r.slice_index)


def check(L, strings, patterns, packed=True, layout="packed", flags=0, misalign=None, rng=None, want_selected=None):
    rng = rng or random.Random(len(strings))
    strings = list(strings)
    offs, arena = lay_out(strings, layout, rng)
    if misalign is not None and strings:
        # the arena ends at a page boundary: the address of its first byte is decided by its length
        pad = ((16 - misalign) - len(arena)) % 16
        if pad:
            strings.append(b"q" * pad); offs.append(len(arena)); arena += b"q" * pad
    n = len(strings)
    region, region_bytes = C.c_void_p(), C.c_uint64()
    base = L.sxs_guarded(max(1, len(arena)), C.byref(region), C.byref(region_bytes))
    assert base
    try:
        C.memmove(base, arena, len(arena))
        if misalign is not None and strings:
            assert base % 16 == misalign
        arr = records(strings, offs, packed)
        pat_bytes = b"".join(p.ljust(64, b"\xEE") for p in patterns)
        pat_len = (C.c_uint32 * len(patterns))(*[len(p) for p in patterns])
        want = [i for i, s in enumerate(strings) if matches(s, patterns, bool(flags & NOCASE)) != bool(flags & INVERT)]
        if want_selected is not None:
            assert want == want_selected, (want, want_selected)     # (the case is what its author meant)
        total = sum(len(strings[i]) for i in want)
        out = ((sx.Finding16 if packed else sx.Finding) * max(1, n))()
        raw = C.create_string_buffer(b"\xEE" * (total + 64), total + 64)
        waves = (n + 63) // 64
        masks = (C.c_uint64 * (waves + 1))()
        n_sel, sel_bytes, range_waves = C.c_uint64(), C.c_uint64(), C.c_uint64()
        rc = L.sxs_select_host(C.addressof(arr), n, int(packed), base, pat_bytes, pat_len, len(patterns), flags, C.addressof(out),
                               C.addressof(raw), total, masks, C.byref(n_sel), C.byref(sel_bytes), C.byref(range_waves))
        assert rc == 0, rc
        got = [w * 64 + b for w in range(waves) for b in range(64) if masks[w] >> b & 1] if n else []
        assert got == want, (sorted(set(got) ^ set(want))[:10], len(got), len(want))
        assert (n_sel.value, sel_bytes.value) == (len(want), total)
        if n:
            assert range_waves.value == (waves if layout == "packed" else range_waves.value)
        out_arena = raw.raw
        assert out_arena[total:] == b"\xEE" * 64, "bytes behind the selected strings were written"
        off = 0
        for k, i in enumerate(want):
            assert fields(out[k], packed) == fields(arr[i], packed), (k, i)           # every record unchanged except str_off
            assert out[k].str_off == off, (k, out[k].str_off, off)                  # back to back, in record order
            assert out_arena[off:off + len(strings[i])] == strings[i], (k, i)
            off += len(strings[i])
        return want, range_waves.value
    finally:
        L.sxs_unmap(region, region_bytes)


def text(rng, n, alphabet=b"abAB \xc3\x84\xa4"):
    return bytes(rng.choice(alphabet) for _ in range(n))


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("layout", ["packed", "scattered"])
def test_every_pattern_length(core, packed, layout):
    rng = random.Random(1)
    strings = [text(rng, rng.choice((3, 10, 20, 64, 65, 100, 150))) for _ in range(200)]
    for ln in range(1, 65):
        src = rng.choice([s for s in strings if len(s) >= ln])
        o = rng.randrange(0, len(src) - ln + 1)
        want, _ = check(core, strings, [src[o:o + ln]], packed, layout, rng=rng)
        assert want
        check(core, strings, [src[o:o + ln - 1] + b"#"], packed, layout, rng=rng, want_selected=[])


@pytest.mark.parametrize("layout", ["packed", "scattered"])
def test_a_hit_at_the_first_and_at_the_last_byte(core, layout):
    strings = [b"needle....", b"....needle", b"..needle..", b"needl", b"eedle", b"needle", b"xneedl", b"e"]
    check(core, strings, [b"needle"], layout=layout, want_selected=[0, 1, 2, 5])
    check(core, [b"e"] * 3 + [b"x", b"xe", b"ex"], [b"e"], layout=layout, want_selected=[0, 1, 2, 4, 5])


def test_a_pattern_that_exists_only_across_two_records_does_not_match(core):
    strings = [b"....ab", b"cd....", b"a", b"b", b"c", b"d", b"", b"abc", b"", b"d"]
    for packed in (True, False):
        check(core, strings, [b"abcd"], packed, want_selected=[])
        check(core, strings, [b"abcd", b"bc"], packed, want_selected=[7])
    # at a wavefront's edge: records 63 and 64
    strings = [b"0123456789"] * 63 + [b"....ab", b"cd....", b"tail"]
    check(core, strings, [b"abcd"], want_selected=[])
    check(core, strings, [b"ab", b"cd"], want_selected=[63, 64])


@pytest.mark.parametrize("misalign", [0, 5])
def test_hits_across_a_chunk_edge_and_a_wavefronts_range_edge(core, misalign):
    """back to back, the arena's first byte `misalign` bytes behind a 16-byte boundary: every string holds the pattern once, at
    every position relative to the chunks; then a pattern that begins in the last chunk of wavefront 0's range"""
    rng = random.Random(5)
    pat = b"NEEDLE7"
    strings = []
    for i in range(200):
        s = bytearray(text(rng, 9 + i % 23, b"abc"))
        at = i % (len(s) - len(pat) + 1)
        s[at:at + len(pat)] = pat
        strings.append(bytes(s))
    want, range_waves = check(core, strings, [pat], misalign=misalign, want_selected=list(range(200)))
    assert range_waves >= 4
    check(core, strings, [pat[:-1] + b"8"], misalign=misalign, want_selected=[])
    # the last record of wavefront 0 ends with the pattern, the first of wavefront 1 begins with it; 62|63 and 64|65 hold it split
    strings = [b"0123456789ab"] * 62 + [b"....NEED", b"LE7.NEEDLE7", b"NEEDLE7.NEED", b"LE7."]
    check(core, strings, [pat], misalign=misalign, want_selected=[63, 64])


def test_self_overlapping_patterns(core):
    strings = [b"aaaa", b"aaa", b"aa", b"baaab", b"ababab", b"abab", b"aba", b"aabaab"]
    check(core, strings, [b"aaa"], want_selected=[0, 1, 3])
    check(core, strings, [b"abab"], want_selected=[4, 5])
    check(core, strings, [b"aabaa"], want_selected=[7])
    check(core, strings, [b"aaa", b"abab"], layout="scattered", want_selected=[0, 1, 3, 4, 5])


@pytest.mark.parametrize("layout", ["packed", "scattered"])
def test_empty_strings_and_strings_shorter_than_the_pattern(core, layout):
    strings = [b"", b"a", b"", b"", b"ab", b"abc", b"", b"abcd", b""] * 20
    check(core, strings, [b"abc"], layout=layout, want_selected=[i for i in range(180) if i % 9 in (5, 7)])
    check(core, strings, [b"abc"], layout=layout, flags=INVERT, want_selected=[i for i in range(180) if i % 9 not in (5, 7)])
    check(core, [b""] * 130, [b"a"], layout=layout, want_selected=[])
    check(core, [b""] * 130, [b"a"], layout=layout, flags=INVERT, want_selected=list(range(130)))


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("n_patterns", [1, 2, 16])
def test_one_two_and_sixteen_patterns(core, n_patterns, packed):
    rng = random.Random(20 + n_patterns)
    strings = [text(rng, rng.randrange(0, 40), b"abcdefgh") for _ in range(1000)]
    patterns = [text(rng, rng.randrange(2, 5), b"abcdefgh") for _ in range(n_patterns)]
    for layout in ("packed", "scattered"):
        want, _ = check(core, strings, patterns, packed, layout, rng=rng)
        assert 0 < len(want) < len(strings)
        for k, p in enumerate(patterns):   # every pattern of the list counts, whatever its place
            only = [i for i, s in enumerate(strings) if p in s]
            assert set(only) <= set(want)
            check(core, strings, [b"#" * 3] * k + [p] + [b"#" * 3] * (n_patterns - 1 - k), packed, layout, rng=rng, want_selected=only)


def test_nocase_folds_ascii_letters_and_nothing_else(core):
    strings = ["Ärger".encode(), "ärger".encode(), "ÄRGER".encode(), b"\xc3\x84RGER", b"\xc3\xa4RGER", b"[rger", b"{RGER", b"@Z`z", b"@z`Z"]
    for layout in ("packed", "scattered"):
        check(core, strings, ["Ärger".encode()], layout=layout, want_selected=[0])
        check(core, strings, ["Ärger".encode()], layout=layout, flags=NOCASE, want_selected=[0, 2, 3])      # C3 84 is not C3 A4
        check(core, strings, ["ärGER".encode()], layout=layout, flags=NOCASE, want_selected=[1, 4])
        check(core, strings, [b"[RGER"], layout=layout, flags=NOCASE, want_selected=[5])                       # '[' = 'Z' + 1, '{' = 'z' + 1
        check(core, strings, [b"@Z`Z"], layout=layout, flags=NOCASE, want_selected=[7, 8])                     # '@' = 'A' - 1, '`' = 'a' - 1
        check(core, strings, [b"RGER"], layout=layout, flags=NOCASE | INVERT, want_selected=[7, 8])
    rng = random.Random(30)
    strings = [text(rng, rng.randrange(0, 30)) for _ in range(500)]
    for pat in (b"aB", b"\xc3\x84a", b"b \xa4", b"ABA"):
        want, _ = check(core, strings, [pat], flags=NOCASE, rng=rng)
        assert want


@pytest.mark.parametrize("packed", [True, False])
def test_invert_and_the_plain_selection_partition_the_records(core, packed):
    rng = random.Random(40)
    strings = [text(rng, rng.randrange(0, 30), b"abc") for _ in range(700)]
    for layout in ("packed", "scattered"):
        a, _ = check(core, strings, [b"abc", b"cc"], packed, layout, rng=rng)
        b, _ = check(core, strings, [b"abc", b"cc"], packed, layout, flags=INVERT, rng=rng)
        assert a and b and sorted(a + b) == list(range(700))


@pytest.mark.parametrize("misalign", range(16))
def test_every_misalignment_of_the_arena(core, misalign):
    rng = random.Random(50 + misalign)
    strings = [text(rng, rng.randrange(0, 40), b"abcd") for _ in range(300)]
    for layout in ("packed", "scattered"):
        want, _ = check(core, strings, [b"abca", b"dd"], layout=layout, misalign=misalign, rng=rng)
        assert 0 < len(want) < 300
        check(core, strings, [b"abcadd"], packed=False, layout=layout, misalign=misalign, rng=rng)


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_record_counts_around_a_wavefront(core, n, packed):
    rng = random.Random(60 + n)
    strings = [text(rng, rng.randrange(0, 24), b"abc") for _ in range(n)]
    for layout in ("packed", "scattered"):
        for flags in (0, INVERT):
            check(core, strings, [b"ab"], packed, layout, flags=flags, rng=rng)
        check(core, strings, [b"#"], packed, layout, rng=rng, want_selected=[])
        check(core, strings, [b"#"], packed, layout, flags=INVERT, rng=rng, want_selected=list(range(n)))
    if n:
        strings[-1] = b"the last one"
        check(core, strings, [b"last one"], packed, want_selected=[n - 1])
        strings[0] = b"the first one"
        check(core, strings, [b"the first"], packed, want_selected=[0])


@pytest.mark.parametrize("packed", [True, False])
def test_a_string_of_16000_bytes(core, packed):
    rng = random.Random(70)
    strings = [text(rng, rng.randrange(4, 24), b"abc") for _ in range(150)]
    big = bytearray(text(rng, 16000, b"abc"))
    big[15990:16000] = b"ENDOFBIG.."
    big[8000:8006] = b"MIDDLE"
    strings[40] = bytes(big)
    strings[41] = bytes(big[:15990]) + b"ENDOFBI"
    strings[149] = bytes(big)
    for layout in ("packed", "scattered"):
        check(core, strings, [b"ENDOFBIG.."], packed, layout, rng=rng, want_selected=[40, 149])
        check(core, strings, [b"MIDDLE"], packed, layout, rng=rng, want_selected=[40, 41, 149])
        check(core, strings, [b"ENDOFBIG..."], packed, layout, rng=rng, want_selected=[])
        check(core, strings, [b"MIDDLE"], packed, layout, flags=INVERT, rng=rng)
