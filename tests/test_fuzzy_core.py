"""Which keywords occur in a string with at most k errors (sx_result_fuzzy_device's rule): the lane functions of
stringsext_amd/csrc/sx_fuzzy_core.hpp as the library runs them on the host, through sx_fuzzy_bytes (stringsext_amd.fuzzy), against
tests/fuzzy_plant.py — Sellers' table restated in Python as include/stringsext_amd.h states it.  No expected value comes from the code
under test.  The same lane functions run once more as a program of their own under the address and undefined-behaviour sanitizers
(tests/native/fuzzy_core_host.cpp), every string in an allocation that ends where it ends; that program also checks the builder's
tables: the class order and the rows that stay out of LDS.  The refusals are the builder's, read through a host-only context."""
import ctypes as C
import os
import subprocess

import pytest

import fuzzy_plant as fz
import refconfig as rc
import stringsext_amd as sx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "stringsext_amd", "csrc")
DEPS = [os.path.join(NATIVE, "fuzzy_core_host.cpp"), os.path.join(ROOT, "include", "stringsext_amd.h")] + [
    os.path.join(CSRC, f) for f in ("sx_fuzzy_core.hpp", "sx_fuzzy_build.hpp", "sx_fuzzy_build.cpp", "sx_label_core.hpp", "sx_measure_core.hpp", "sx_select_core.hpp")]
G32, G64 = 8, 4      # kFuzzyGroup32, kFuzzyGroup64 (test_the_groups_are_the_sources)


def check(patterns, ks, s, nocase=False):
    got, want = sx.fuzzy(patterns, ks, s, nocase), fz.word(patterns, ks, s, nocase)
    assert got == want, (len(patterns), ks, s[:80], hex(got), hex(want))
    return got


def test_the_groups_are_the_sources():
    from test_gpu_result_strides import constant
    assert (constant("kFuzzyGroup32"), constant("kFuzzyGroup64")) == (G32, G64)
    assert (sx.SX_FUZZY_MAX_PATTERNS, sx.SX_FUZZY_MAX_PATTERN_BYTES, sx.SX_FUZZY_MAX_ERRORS) == (64, 64, 8)
    assert sx.lib().sx_abi_version() == 4 and {"sx_fuzzy_set_create", "sx_result_fuzzy_device", "sx_fuzzy_bytes"} <= set(sx.EXPORTS)


@pytest.mark.parametrize("m", fz.LENGTHS)
def test_every_length_budget_and_alphabet_with_variants_at_k_and_k_plus_1(m):
    for symbols in fz.ALPHABETS:      # (256: bytes of 0x80 and above in pattern and string — a sign-extended byte would show)
        p = fz.made(m, symbols, m + symbols)
        for k in fz.legal_ks(m):
            # texts of length 0, len - k - 1, len - k, len, and long: the pattern's own prefix, and other text
            for n in (0, m - k - 1, m - k, m, 500):
                check([p], k, p[:n] + fz.made(max(0, n - m), symbols, n))
                check([p], k, fz.made(n, symbols, n + 1))
            assert sx.fuzzy([p], k, p[:m - k]) == 1 and sx.fuzzy([p], k, p[:m - k - 1]) == 0
            for e in (k, k + 1):
                text, v = fz.variant(p, e, seed=k)
                assert check([p], k, text) == (1 if e == k else 0)
                if symbols < 256:      # (the filler holds no byte of the pattern) at the head, in the middle, as the tail
                    for where in ("head", "middle", "tail"):
                        assert check([p], k, fz.placed(v, where, 90, e)) == (1 if e == k else 0), (m, k, e, where)


def test_each_edit_kind_at_the_first_and_the_last_pattern_byte():
    for m in (2, 31, 32, 33, 63, 64):
        p = fz.made(m, 26, m)
        for kind in "sid":
            for seed in (0, 1):
                s = b"QQQ " + fz.edited(p, 1, seed, kinds=kind) + b" QQQ"
                assert check([p], 1 if m > 1 else 0, s) == 1 and (m < 3 or check([p], 0, s) == 0), (m, kind, seed)


def test_no_errors_is_the_substring():
    for m in (1, 2, 5, 32, 33, 64):
        for symbols in (2, 4, 26):
            p = fz.made(m, symbols, m)
            for n in range(0, 200, 7):
                t = fz.made(n, symbols, n) + (p if n % 3 == 0 else b"")+ fz.made(n % 5, symbols, 1)
                assert sx.fuzzy([p], 0, t) == (1 if p in t else 0), (m, symbols, n)


def test_the_case_union_folds_a_to_z_in_pattern_and_string_and_nothing_else():
    assert check([b"PassWord"], 1, b"xx pAssw0RD yy", True) == 1 and check([b"PassWord"], 1, b"xx pAssw0RD yy", False) == 0
    assert check([b"a[b"], 0, b"A{B", True) == 0 and check([b"a[b"], 0, b"A[B", True) == 1                      # '[' | 0x20 == '{'
    assert check(["Ж".encode()], 0, "ж".encode(), True) == 0 and check(["é".encode()], 0, "É".encode(), True) == 0
    pats, ks, nocase = fz.SETS["nocase"]
    for s in fz.lines(300):
        check(pats, ks, s, nocase)
        check(pats, ks, s.upper(), nocase)


@pytest.mark.parametrize("n", (1, G64 - 1, G64, G64 + 1, G32 - 1, G32, G32 + 1, 63, 64))
@pytest.mark.parametrize("longest", (12, 40))
def test_sets_around_a_group_and_up_to_bit_63(n, longest):
    """longest = 12: the 32-bit words and groups of G32; 40: the 64-bit words and groups of G64"""
    pats = [fz.made(2 + (p * 7 + n) % (longest - 1), 26, p + 100 * n) for p in range(n)]
    pats[-1] = fz.made(longest, 26, n)
    ks = [min(len(x) - 1, p % 4) for p, x in enumerate(pats)]
    seen = 0
    for t in range(60):
        s = fz.made(t % 9, 26, t) + b"".join(fz.edited(pats[fz.mix(t * 13 + j) % n], min(2, len(pats[fz.mix(t * 13 + j) % n])), t) + fz.made(3 + j, 26, t + j) for j in range(1 + t % 3))
        seen |= check(pats, ks, s)
    seen |= check(pats, ks, b"".join(pats))
    assert seen == (1 << n) - 1 and check(pats, ks, b"") == 0                                               # every bit was set once, bit n - 1 too


def test_the_planted_sets_over_the_planted_lines():
    ls = fz.lines(150)
    for name, (pats, ks, nocase) in fz.SETS.items():
        for s in ls[:150 if len(pats) < 64 else 60]:      # (sx_fuzzy_bytes compiles the set on every call)
            check(pats, ks, s, nocase)
    pats, ks, _ = fz.SETS["many"]      # the rows beyond the LDS share, with matches
    assert check(pats, ks, b"xx passw0rd administrat0r") == 3


def test_a_long_string_with_the_match_in_its_last_bytes():
    pats, ks = fz.LONG_SET
    stem = ("\U00020000" * 15998).encode()
    for tail in (fz.LONG_TAIL, fz.LONG_TAIL[4:] + fz.LONG_TAIL[:4], b"limit last lane"):
        assert check(pats, ks, stem + tail) != 0 and check(pats, ks, stem + tail[:-3]) in (0, 8)


def refusal(host, patterns, ks, flags=0):
    arr, n = sx._pattern_array(patterns)
    out = C.c_void_p(0xDEAD0)
    rc_ = sx.lib().sx_fuzzy_set_create(host.h, arr, bytes(ks), n, flags, C.byref(out))
    word = C.c_uint64(77)
    assert sx.lib().sx_fuzzy_bytes(arr, bytes(ks), n, flags, b"abc", 3, C.byref(word)) == (sx.SX_E_INVALID if rc_ == sx.SX_E_INVALID else sx.SX_OK)
    assert out.value is None and (rc_ != sx.SX_E_INVALID or word.value == 0)
    return rc_, sx.lib().sx_last_error(host.h).decode()


def test_every_refusal_with_its_text_and_a_host_only_context():
    host = sx.Scanner(rc.missions(encodings=["utf-8"]), device=sx.SX_HOST_ONLY)
    try:
        ok = [b"abc"] * 3
        for patterns, ks, flags, text in (
                (ok[:2] + [b""], [0, 0, 0], 0, "fuzzy set: pattern 2: an empty pattern"),
                ([b"ab", b"x" * 65], [0, 0], 0, "fuzzy set: pattern 1: 65 bytes, and a pattern has at most 64"),
                ([b"x" * 64, b"y" * 20, b"abc"], [8, 9, 0], 0, "fuzzy set: pattern 1: 9 errors, and a budget is at most 8"),
                (ok, [2, 2, 3], 0, "fuzzy set: pattern 2: 3 errors for 3 bytes: the budget must be smaller than the length"),
                ([b"a"], [1], 0, "fuzzy set: pattern 0: 1 errors for 1 bytes: the budget must be smaller than the length"),
                ([b"ab"] * 65, [0] * 65, 0, "fuzzy set: n_patterns must be 1..64"),
                (ok, [0, 0, 0], sx.SX_SELECT_INVERT, "fuzzy set: a fuzzy set takes SX_SELECT_ASCII_NOCASE and no other flag"),
                (ok, [0, 0, 0], 0x80000000, "fuzzy set: a fuzzy set takes SX_SELECT_ASCII_NOCASE and no other flag")):
            assert refusal(host, patterns, ks, flags) == (sx.SX_E_INVALID, text)
        L = sx.lib()
        out = C.c_void_p(0xDEAD0)
        arr, n = sx._pattern_array(ok)
        assert L.sx_fuzzy_set_create(host.h, arr, b"\0\0\0", 0, 0, C.byref(out)) == sx.SX_E_INVALID and out.value is None      # no pattern
        assert L.sx_fuzzy_set_create(host.h, arr, None, 3, 0, C.byref(out)) == sx.SX_E_INVALID
        assert L.sx_fuzzy_set_create(host.h, arr, b"\0\0\0", 3, 0, None) == sx.SX_E_INVALID
        # what is legal is compiled, and then there is no device for it
        rc_, text = refusal(host, [b"x" * 64, b"a"], [8, 0], sx.SX_SELECT_ASCII_NOCASE)
        assert rc_ == sx.SX_E_STATE and "host-only" in text
        with pytest.raises(sx.SxError) as e:
            host.fuzzy_set([b"abc", b"de"], max_errors=[1, 2])
        assert e.value.code == sx.SX_E_INVALID and "pattern 1" in str(e.value)
        with pytest.raises(ValueError):
            host.fuzzy_set([b"abc", b"de"], max_errors=[1])
        # sx_fuzzy_bytes' own: pointers and the length
        word = C.c_uint64(77)
        assert L.sx_fuzzy_bytes(arr, b"\0\0\0", 3, 0, None, 0, C.byref(word)) == sx.SX_OK and word.value == 0
        assert L.sx_fuzzy_bytes(arr, b"\0\0\0", 3, 0, None, 3, C.byref(word)) == sx.SX_E_INVALID
        assert L.sx_fuzzy_bytes(arr, b"\0\0\0", 3, 0, b"abc", 3, None) == sx.SX_E_INVALID
        assert L.sx_fuzzy_bytes(arr, b"\0\0\0", 3, 0, b"abc", 1 << 32, C.byref(word)) == sx.SX_E_INVALID and word.value == 0
        assert L.sx_fuzzy_set_info_get(None, None) == sx.SX_E_INVALID and L.sx_fuzzy_set_reset(None) == sx.SX_E_INVALID
        assert L.sx_fuzzy_set_read(None, None, None, 0) == sx.SX_E_INVALID and L.sx_fuzzy_set_counters_device(None, None, None) == sx.SX_E_INVALID
        L.sx_fuzzy_set_free(None)
    finally:
        host.close()
    assert sx.fuzzy([b"abc"], 0, b"xabcx") == 1 and sx.fuzzy([b"abc"], [0], b"") == 0


# ---- the same lane functions under the address and undefined-behaviour sanitizers, as a program of their own

def test_a_sanitizer_build_matches_the_same():
    exe, src = os.path.join(NATIVE, "fuzzy_core_main"), os.path.join(NATIVE, "fuzzy_core_host.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in DEPS):
        tmp = f"{exe}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", tmp, src])
        os.replace(tmp, exe)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("fuzzy core: ok"), (out.stdout[-500:], out.stderr[-2000:])
