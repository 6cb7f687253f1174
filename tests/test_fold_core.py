"""Unicode simple case folding (SX_FOLD_SIMPLE): the lane functions of stringsext_amd/csrc/sx_fold_core.hpp as the library runs them
on the host, through sx_fold_utf8 (stringsext_amd.fold), against Python — str.casefold() and str.lower() per character as the rule
is stated, and the `surrogateescape` decoder for what is no well-formed UTF-8.  No expected value comes from the code under test.
The same lane functions run once more as a program of their own under the address and undefined-behaviour sanitizers
(tests/native/fold_core_host.cpp), every input and output in an allocation that ends where it ends."""
import ctypes as C
import os
import re
import subprocess
import unicodedata

import pytest

import stringsext_amd as sx
from fold_plant import fold, fold_char

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "stringsext_amd", "csrc")
TABLE = os.path.join(CSRC, "sx_fold_table.inc")
DEPS = [os.path.join(NATIVE, "fold_core_host.cpp"), os.path.join(ROOT, "include", "stringsext_amd.h"), TABLE] + [
    os.path.join(CSRC, f) for f in ("sx_fold_core.hpp", "sx_order_core.hpp", "sx_label_core.hpp", "sx_select_core.hpp")]
SCALARS = [c for c in range(0x110000) if not 0xD800 <= c <= 0xDFFF]


def table_text():
    with open(TABLE) as f:
        return f.read()


def committed_pairs():
    """{from: to}: the pair list of the committed table"""
    body = re.search(r"kFoldPairs\[kFoldPairCount\]\[2\] = \{(.*?)\n\};", table_text(), re.S).group(1)
    return {int(a, 16): int(b, 16) for a, b in re.findall(r"\{ 0x([0-9A-F]+), 0x([0-9A-F]+) \}", body)}


def table_version():
    return re.search(r'#define SX_FOLD_UNIDATA_VERSION "([0-9.]+)"', table_text()).group(1)


@pytest.fixture(scope="module")
def fold_one():
    """bytes -> bytes through sx_fold_utf8, one call into a buffer kept for the module: a code point at a time is a million calls"""
    L = sx.lib()
    out, n = C.create_string_buffer(256), C.c_uint64()

    def call(b):
        rc = L.sx_fold_utf8(b, len(b), sx.SX_FOLD_SIMPLE, out, 256, C.byref(n))
        assert rc == sx.SX_OK, (rc, b)
        return out.raw[:n.value]
    return call


def test_the_committed_table_is_the_generators_and_has_the_numbers_the_rule_names():
    pairs = committed_pairs()
    assert len(pairs) == 1414 and max(pairs) == 0x1E921 and all(t not in pairs for t in pairs.values())
    assert pairs[0x212A] == ord("k") and pairs[0x1E9E] == 0xDF and pairs[0x3C2] == 0x3C3 and 0xDF not in pairs and 0x130 not in pairs
    if unicodedata.unidata_version != table_version():
        pytest.skip("the table is of Unicode %s, this Python's unicodedata of %s: the formula is not compared" % (table_version(), unicodedata.unidata_version))
    want = {c: ord(fold_char(chr(c))) for c in SCALARS if fold_char(chr(c)) != chr(c)}
    assert pairs == want


def test_every_code_point_singly(fold_one):
    pairs = committed_pairs()
    same_version = unicodedata.unidata_version == table_version()
    bad = []
    for c in SCALARS:
        want = fold_char(chr(c)) if same_version else chr(pairs.get(c, c))
        if fold_one(chr(c).encode()) != want.encode():
            bad.append(hex(c))
    assert not bad, (len(bad), bad[:20])
    if not same_version:
        pytest.skip("checked against the committed pair list of Unicode %s; this Python's unicodedata is of %s and was not compared" % (table_version(), unicodedata.unidata_version))


def test_the_fold_is_idempotent_over_every_code_point(fold_one):
    bad = []
    for c in SCALARS:
        once = fold_one(chr(c).encode())
        if fold_one(once) != once:
            bad.append(hex(c))
    assert not bad, (len(bad), bad[:20])


def test_all_two_byte_strings_against_surrogateescape(fold_one):
    bad = [(a, b) for a in range(256) for b in range(256) if fold_one(bytes((a, b))) != fold(bytes((a, b)))]
    assert not bad, (len(bad), bad[:20])


SECONDS, THIRDS = (0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0), (0x7F, 0x80, 0xBF, 0xC0)


def edge_vectors():
    """every lead byte with 0 to 3 bytes behind it from the edges of Table 3-7 — E0 9F/A0, ED 9F/A0, F0 8F/90, F4 8F/90, and with them
    C0, C1 and F5..FF as leads —, each whole in front of a letter and cut short by the end of the string"""
    out = []
    for lead in range(0x80, 0x100):
        tails = [b""] + [bytes((x,)) for x in SECONDS] + [bytes((x, y)) for x in SECONDS for y in THIRDS] + [bytes((x, y, z)) for x in SECONDS for y in THIRDS for z in THIRDS]
        for t in tails:
            s = bytes((lead,)) + t
            out += [s, s + b"Z", b"A" + s]
    return out


def test_the_edges_of_table_3_7_whole_and_cut_short(fold_one):
    vectors = edge_vectors()
    for s in (b"\xe0\x9f\x80", b"\xe0\xa0\x80", b"\xed\x9f\xbf", b"\xed\xa0\x80", b"\xf0\x8f\x80\x80", b"\xf0\x90\x80\x80", b"\xf4\x8f\xbf\xbf", b"\xf4\x90\x80\x80",
              b"\xc0\x80", b"\xc1\xbf", b"\xf5\x80\x80\x80", b"\xff", b"\xe2\x80", b"\xf0\x90\x80"):
        assert s in vectors
    bad = [s for s in vectors if fold_one(s) != fold(s)]
    assert not bad, (len(bad), bad[:20])
    # a well-formed sequence keeps its bytes or folds; an ill-formed one is copied byte for byte
    assert fold_one(b"\xed\xa0\x80") == b"\xed\xa0\x80" and fold_one(b"\xe2\x84") == b"\xe2\x84" and fold_one(b"\xe2\x84\xaa") == b"k"
    assert fold_one(b"\xc3A\xc3\x84") == b"\xc3a\xc3\xa4"


WORD_CHARS = ["П", "é", "\u023A", "\u023E", "\u212A", "\u1E9E", "\U00010400", "漢", "ß"]      # keeps its length, grows (2), shrinks (2), four bytes, stays (2)


def test_the_word_path_at_every_alignment_with_a_character_at_every_offset():
    L = sx.lib()
    assert any(len(fold(c.encode())) > len(c.encode()) for c in WORD_CHARS) and any(len(fold(c.encode())) < len(c.encode()) for c in WORD_CHARS)
    page = C.create_string_buffer(4096 + 64)
    base = (C.addressof(page) + 63) // 64 * 64
    out, n = C.create_string_buffer(64), C.c_uint64()
    first = last = 0
    for alignment in range(8):
        for length in range(26):
            ascii_ = bytes(0x41 + (i * 7 + length) % 26 for i in range(length))
            cases = [ascii_]
            for ch in WORD_CHARS:
                e = ch.encode()
                cases += [ascii_[:at] + e + ascii_[at + len(e):] for at in range(length - len(e) + 1)]
            for s in cases:
                C.memmove(base + alignment, s, len(s))
                # a byte >= 0x80 at the first and at the last byte of an 8-byte word
                first += any(b >= 0x80 and (alignment + i) % 8 == 0 for i, b in enumerate(s))
                last += any(b >= 0x80 and (alignment + i) % 8 == 7 for i, b in enumerate(s))
                rc = L.sx_fold_utf8(C.cast(base + alignment, C.c_char_p), len(s), 0, out, 64, C.byref(n))
                assert rc == sx.SX_OK and out.raw[:n.value] == fold(s), (alignment, s, out.raw[:n.value])
    assert first > 100 and last > 100


def test_a_long_string_of_every_script():
    s = ("PASSWORD ПАРОЛЬ Straße STRASSE ÅNGSTRÖM ΑΘΉΝΑ οδυσσεύς \u212Aelvin \u023A\u023E \u1E9E \u0130stanbul 漢字 ᏣᎳᎩ ꮃꭳꭹ \U00010400\U00010428 " * 40).encode()
    assert sx.fold(s) == fold(s) and len(sx.fold(s)) != len(s)
    assert sx.fold(b"") == b"" and sx.fold("ПАРОЛЬ".encode()) == "пароль".encode() and sx.fold("Straße".encode()) == "straße".encode()
    assert sx.fold("ΑΘΉΝΑ".encode()) == sx.fold("Αθήνα".encode()) and sx.fold("ÅNGSTRÖM".encode()) == "ångström".encode()


def test_the_size_query_a_capacity_one_too_small_and_an_unknown_flag():
    L = sx.lib()
    s = "\u023A\u023E ПАРОЛЬ k".encode()            # grows: 2 more bytes than it had
    want = fold(s)
    assert len(want) == len(s) + 2
    n = C.c_uint64(77)
    assert L.sx_fold_utf8(s, len(s), 0, None, 0, C.byref(n)) == sx.SX_OK and n.value == len(want)
    out = C.create_string_buffer(b"\xEE" * 64, 64)
    n = C.c_uint64(77)
    assert L.sx_fold_utf8(s, len(s), 0, out, len(want) - 1, C.byref(n)) == sx.SX_E_INVALID
    assert n.value == len(want) and out.raw == b"\xEE" * 64                     # refused: what is needed, and nothing written
    assert L.sx_fold_utf8(s, len(s), 0, out, len(want), C.byref(n)) == sx.SX_OK
    assert n.value == len(want) and out.raw[:len(want)] == want and out.raw[len(want):] == b"\xEE" * (64 - len(want))      # nothing behind cap
    n = C.c_uint64(77)
    for flags in (1, 2, 0x80000000):
        assert L.sx_fold_utf8(s, len(s), flags, out, 64, C.byref(n)) == sx.SX_E_INVALID and n.value == 0
    assert L.sx_fold_utf8(s, len(s), 0, out, 64, None) == sx.SX_E_INVALID
    assert L.sx_fold_utf8(None, 0, 0, out, 64, C.byref(n)) == sx.SX_OK and n.value == 0
    assert sx.lib().sx_abi_version() == 4 and {"sx_fold_utf8", "sx_result_fold_device", "sx_labels_rebind"} <= set(sx.EXPORTS)


# ---- the same lane functions under the address and undefined-behaviour sanitizers, as a program of their own

def test_a_sanitizer_build_folds_the_same():
    exe, src = os.path.join(NATIVE, "fold_core_main"), os.path.join(NATIVE, "fold_core_host.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in DEPS):
        tmp = f"{exe}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", tmp, src])
        os.replace(tmp, exe)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("fold core: ok"), (out.stdout[-500:], out.stderr[-2000:])
