"""What a string looks like (sx_result_measure_device's rule): the lane functions of stringsext_amd/csrc/sx_measure_core.hpp as the
library runs them on the host, through sx_measure_bytes (stringsext_amd.measure), against tests/measure_plant.py — the rule restated
in Python as include/stringsext_amd.h states it — and against Shannon's formula in floating point.  No expected value comes from the
code under test.  The same lane functions run once more as a program of their own under the address and undefined-behaviour
sanitizers (tests/native/measure_core_host.cpp), every string and counter block in an allocation that ends where it ends.

The bound against floating point, 2^-12 + 2^-15 bits per byte, is derived: ENT is floored to units of 2^-12 (an error in [0, 2^-12)),
and T / n = LG(n) - sum(c/n x LG(c)) in units of 2^-16, where every LG lies at most 1.00001 units below log2 and never above it: both
sides of the difference are weighted means of such errors, so T / n is off by at most 1.00001 x 2^-16 either way — well inside
2^-15."""
import ctypes as C
import os
import subprocess

import pytest

import measure_plant as mp
import stringsext_amd as sx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "stringsext_amd", "csrc")
DEPS = [os.path.join(NATIVE, "measure_core_host.cpp"), os.path.join(ROOT, "include", "stringsext_amd.h")] + [
    os.path.join(CSRC, f) for f in ("sx_measure_core.hpp", "sx_select_core.hpp")]
BOUND = 2.0 ** -12 + 2.0 ** -15
ALPHABETS = {1: b"\xc3", 2: b"aB", 16: b"0123456789abcdef", 64: bytes(range(0x30, 0x70)), 256: bytes(range(256))}


def made(n, symbols):
    """n bytes over an alphabet of `symbols` values, a function of (n, symbols): a linear congruence from the index, no random state"""
    alphabet, x, out = ALPHABETS[symbols], (n * 2654435761 + symbols * 40503) & 0xFFFFFFFF, bytearray(n)
    for i in range(n):
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = alphabet[(x >> 24) % symbols]
    return bytes(out)


def check(s):
    """sx_measure_bytes(s) is the restatement's word, and its entropy field is Shannon's within the derived bound"""
    got, want = sx.measure(s), mp.measure(s)
    assert got == want, (len(s), s[:40], hex(got), hex(want))
    assert abs((got & 0xFFFF) / 4096 - mp.entropy(s)) <= BOUND, (len(s), s[:40], (got & 0xFFFF) / 4096, mp.entropy(s))
    return got


def test_lg_is_monotone_exact_at_powers_of_two_and_just_below_log2():
    """the first half checks the ORACLE, measure_plant.lg16, against math.log2 — what the derived bound rests on —; the second half
    the library's LG against it, on strings whose entropy field isolates it"""
    import math
    last = 0
    for x in list(range(1, 70000)) + [(1 << 32) - 1, 1 << 31, (1 << 31) - 1, 3 << 30]:
        v = mp.lg16(x)
        assert 0 <= math.log2(x) * 65536 - v < 1.00001, x
        if x < 70000:
            assert v >= last
            last = v
    assert [mp.lg16(1 << k) for k in range(32)] == [k << 16 for k in range(32)]
    # n different bytes: T = n x LG(n), so ENT = LG(n) / 16 — the table's entries, through the library
    for n in range(1, 257):
        assert sx.measure(bytes(range(n))) & 0xFFFF == min(65535, mp.lg16(n) // 16), n
    # one byte c times and another once: T = (c + 1) x LG(c + 1) - c x LG(c) — above 255 the library squares at run time
    for c in (1, 2, 3, 254, 255, 256, 257, 1000, 65535, 65536, 1 << 20):
        want = ((c + 1) * mp.lg16(c + 1) - c * mp.lg16(c)) // (16 * (c + 1))
        assert sx.measure(b"a" * c + b"b") & 0xFFFF == want, c


def test_every_single_byte():
    seen = 0
    for b in range(256):
        w = check(bytes([b]))
        cls = mp.byte_class(b)
        assert w == cls | 1 << mp.DISTINCT_SHIFT | (0 if 0x80 <= b <= 0xBF else 1) << mp.CHARS_SHIFT, (b, hex(w))
        seen |= cls
    assert seen == sum(mp.CLASS_NAMES)
    assert mp.byte_class(0x09) == mp.SPACE and mp.byte_class(0x7F) == mp.CONTROL and mp.byte_class(0x0A) == mp.CONTROL and mp.byte_class(0x7E) == mp.PUNCT
    assert mp.byte_class(0x80) == mp.HIGH and mp.byte_class(0x40) == mp.PUNCT and mp.byte_class(0x5B) == mp.PUNCT and mp.byte_class(0x60) == mp.PUNCT


@pytest.mark.parametrize("symbols", sorted(ALPHABETS))
def test_every_length_to_300_over_an_alphabet(symbols):
    for n in range(1, 301):
        w = check(made(n, symbols))
        assert (w >> mp.DISTINCT_SHIFT) & 0x1FF <= min(n, symbols)


def test_one_byte_255_256_and_257_times_alone_and_beside_255_other_values():
    others = bytes(b for b in range(256) if b != ord("x"))
    for n in (255, 256, 257):
        assert check(b"x" * n) == mp.LOWER | 1 << mp.DISTINCT_SHIFT | n << mp.CHARS_SHIFT
        w = check(b"x" * n + others)
        assert (w >> mp.DISTINCT_SHIFT) & 0x1FF == 256 and w & 0xFFFF > 0
        check(others[:100] + b"x" * n + others[100:])


def test_all_256_values_k_times():
    for k in (1, 2, 3, 255, 256, 257):
        w = check(bytes(range(256)) * k)
        assert w & 0xFFFF == 32768 and (w >> mp.DISTINCT_SHIFT) & 0x1FF == 256 and w >> mp.CHARS_SHIFT == 192 * k


def test_long_strings_around_2_16_and_at_2_20():
    for n in (65535, 65536, 65537, 1 << 20):
        check(made(n, 64))
        assert check(b"7" * n) == mp.DIGIT | 1 << mp.DISTINCT_SHIFT | n << mp.CHARS_SHIFT


def test_the_known_answers_of_the_header():
    for s, ent, distinct in ((b"aaaa", 0, 1), (b"abab", 4096, 2), (b"0123456789abcdef", 16384, 16), (bytes(range(256)), 32768, 256)):
        w = check(s)
        assert (w & 0xFFFF, (w >> 16) & 0x1FF) == (ent, distinct), (s[:16], hex(w))
    assert sx.measure("Жé漢\U00010400 a".encode()) >> 32 == 6
    assert sx.SX_MEASURE_ENTROPY_SHIFT == 0 and sx.SX_MEASURE_DISTINCT_SHIFT == 16 and sx.SX_MEASURE_CHARS_SHIFT == 32
    assert [sx.SX_MEASURE_LOWER, sx.SX_MEASURE_UPPER, sx.SX_MEASURE_DIGIT, sx.SX_MEASURE_SPACE, sx.SX_MEASURE_PUNCT, sx.SX_MEASURE_CONTROL,
            sx.SX_MEASURE_HIGH] == [1 << k for k in range(25, 32)] == list(mp.CLASS_NAMES)


def test_every_alignment_of_an_8_byte_word():
    L = sx.lib()
    page = C.create_string_buffer(4096 + 64)
    base = (C.addressof(page) + 63) // 64 * 64
    word = C.c_uint64()
    for alignment in range(8):
        for n in list(range(0, 40)) + [254, 255, 256, 257, 600]:
            s = made(n, 256 if n % 2 else 64)
            C.memmove(base + alignment, s, n)
            assert L.sx_measure_bytes(C.cast(base + alignment, C.c_char_p), n, 0, C.byref(word)) == sx.SX_OK
            assert word.value == mp.measure(s), (alignment, n)


def test_the_empty_string_and_the_refusals():
    L = sx.lib()
    word = C.c_uint64(77)
    assert sx.measure(b"") == 0 == mp.measure(b"")
    assert L.sx_measure_bytes(None, 0, 0, C.byref(word)) == sx.SX_OK and word.value == 0
    for flags in (1, 2, 0x80000000):
        word = C.c_uint64(77)
        assert L.sx_measure_bytes(b"abc", 3, flags, C.byref(word)) == sx.SX_E_INVALID and word.value == 0
    assert L.sx_measure_bytes(b"abc", 3, 0, None) == sx.SX_E_INVALID
    assert L.sx_measure_bytes(None, 3, 0, C.byref(word)) == sx.SX_E_INVALID
    assert L.sx_measure_bytes(b"abc", 1 << 32, 0, C.byref(word)) == sx.SX_E_INVALID            # (refused by its length: no byte is read)
    assert L.sx_measure_bytes(b"abc", (1 << 64) - 1, 0, C.byref(word)) == sx.SX_E_INVALID
    assert sx.lib().sx_abi_version() == 4 and {"sx_result_measure_device", "sx_measure_bytes"} <= set(sx.EXPORTS)


# ---- the same lane functions under the address and undefined-behaviour sanitizers, as a program of their own

def test_a_sanitizer_build_measures_the_same():
    exe, src = os.path.join(NATIVE, "measure_core_main"), os.path.join(NATIVE, "measure_core_host.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in DEPS):
        tmp = f"{exe}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", tmp, src])
        os.replace(tmp, exe)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("measure core: ok"), (out.stdout[-500:], out.stderr[-2000:])
