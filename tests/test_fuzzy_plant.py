"""tests/fuzzy_plant.py holds what its users count on (no GPU, nothing of the product): last_row() is Sellers' table, the variants lie
at exactly the distances they are named for, and in the lines of every source of tests/test_gpu_fuzzy_device.py — as the ORACLE finds
them — every planted pattern's bit is both set and clear somewhere."""
import numpy as np
import pytest

import fold_plant as fp
import fuzzy_plant as fz
import long_plant as lp
import result_plant as rp


def table(p, t):
    """Sellers' table, cell by cell"""
    m = len(p)
    prev, best = list(range(m + 1)), m
    for c in t:
        cur = [0] * (m + 1)
        for i in range(1, m + 1):
            cur[i] = min(prev[i - 1] + (p[i - 1] != c), prev[i] + 1, cur[i - 1] + 1)
        prev, best = cur, min(best, cur[m])
    return best


def test_last_row_is_sellers_table_cell_by_cell():
    k = 0
    for m in (1, 2, 3, 7, 31, 32, 33, 63, 64):
        for symbols in fz.ALPHABETS:
            p = fz.made(m, symbols, m)
            texts = [fz.made(n, symbols, n + m) for n in (0, 1, m - 1, m, m + 1, 90)] + [fz.edited(p, e, m) for e in range(min(m, 9) + 1)]
            assert fz.last_row(p, texts).tolist() == [table(p, t) for t in texts], (m, symbols)      # all texts of a call at once
            assert [fz.distance(p, t) for t in texts] == [table(p, t) for t in texts]                  # and one by one
            k += len(texts)
    assert k > 400
    assert fz.distance(b"abc", b"") == 3 and fz.distance(b"abc", b"xxabcxx") == 0 and fz.distance(b"abc", b"xxabxx") == 1
    assert fz.distance(b"ABC", b"xabcx") == 3 and fz.distance(b"ABC", b"xabcx", True) == 0 and fz.distance("Ж".encode(), "ж".encode(), True) == 1
    assert fz.distance("пароль".encode(), "пороль".encode()) == 1 and fz.distance("пароль".encode(), "парёль".encode()) == 2      # bytes, not characters


@pytest.mark.parametrize("m", fz.LENGTHS)
def test_a_variant_at_exactly_k_and_one_at_exactly_k_plus_1_errors_for_every_length_and_budget(m):
    for symbols in fz.ALPHABETS:
        p = fz.made(m, symbols, m + symbols)
        for k in fz.legal_ks(m):
            for e in (k, k + 1):
                text, v = fz.variant(p, e, seed=k)
                assert table(p, text) == e and v in text, (m, symbols, k, e)
                assert fz.word([p], [k], text) == (1 if e <= k else 0)


def test_each_edit_kind_at_the_first_and_the_last_byte_costs_one():
    for m in (2, 31, 32, 33, 63, 64):
        p = fz.made(m, 26, m)
        seen = set()
        for kind in "sid":
            for seed in (0, 1):      # the first byte, the last byte
                v = fz.edited(p, 1, seed, kinds=kind)
                assert len(v) == m + {"s": 0, "i": 1, "d": -1}[kind] and (v[0] != p[0]) == (seed == 0 and kind != "i")
                assert table(p, b"QQQ " + v + b" QQQ") == 1, (m, kind, seed)
                seen.add(v)
        assert len(seen) == 6


def test_words_puts_pattern_p_into_bit_p_and_memoises():
    pats, ks = fz.SETS["sixty-four"][:2]
    assert len(pats) == 64 and pats[63] == fz.WORDS[0]
    w = fz.words(pats, ks, [b"xx passw0rd", b"nothing"])
    assert int(w[0]) >> 63 == 1 and int(w[0]) & 1 == 1 and int(w[1]) >> 63 == 0
    assert fz.word([b"ab", b"cd"], 0, b"xcdx") == 2 and fz.word([b"ab", b"cd"], [1, 0], b"xcdx a") == 3
    assert (tuple(pats), tuple(ks), False) in fz._memo and b"nothing" in fz._memo[tuple(pats), tuple(ks), False]


def bits(strs, name):
    pats, ks, nocase = fz.SETS[name]
    w = fz.words(pats, ks, strs, nocase)
    return [int(((w >> np.uint64(p)) & np.uint64(1)).sum()) for p in range(len(pats))]


def oracle_strs(ms, data):
    return rp.expected(ms, data).strs


@pytest.mark.parametrize("k", (1, 63, 64, 65, 129))
def test_the_small_sources_hold_one_finding_a_line_and_both_answers(k):
    strs = oracle_strs(fp.ms1(), lp.buffer(fz.lines(k)))
    assert strs == fz.lines(k)
    if k > 1:
        assert all(0 < b < k for b in bits(strs, "five")[:4]), bits(strs, "five")
        assert all(0 < b < k for b in bits(strs, "one"))
    if k >= 129:
        assert all(0 < b < k for b in bits(strs, "nine") + bits(strs, "five")), k
    # strings shorter than len - k beside ones of exactly len - k
    assert fz.lines(4)[:2] == [fz.SHORT, fz.SHORT[:-1]] and len(fz.SHORT) == len(fz.WORDS[0]) - fz.WORD_KS[0]
    assert fz.word(*fz.SETS["one"][:2], fz.SHORT) == 1 and fz.word(*fz.SETS["one"][:2], fz.SHORT[:-1]) == 0


def test_the_merged_source_holds_both_answers_for_every_set():
    strs = oracle_strs(fp.ms2(), lp.buffer(fz.lines(fz.MERGED_LINES)))
    assert len(strs) > 2048 + 1024                     # three parts of 1024 findings and more
    for name in ("one", "nine", "five", "exact", "sixty-four"):
        assert all(0 < b < len(strs) for b in bits(strs, name)), (name, bits(strs, name))
    got = bits(strs, "nocase")
    assert got[2] == 0 and all(0 < b < len(strs) for b in got[:2] + got[3:])      # 'ПАРОЛЬ' is not 'пароль': no byte but A..Z is folded
    assert got[0] > bits(strs, "one")[0] and got[3] > bits(strs, "nine")[3]                # 'PASSW0RD', 'KERNEL32.DLL': some lines hold the other case
    many = bits(strs, "many")
    assert all(0 < b < len(strs) for b in many[:3]) and not any(many[3:])


def test_the_many_classes_set_has_more_classes_than_rows_in_lds_and_the_words_letters_are_the_rarest():
    pats = fz.many_classes()
    held = {}
    for p in pats:
        for x in p:
            held[x] = held.get(x, 0) + 1
    order = sorted(held, key=lambda x: (-held[x], x))
    lds = 48 * 1024 // (64 * 8)
    assert len(pats) == 64 and len(held) + 1 > lds
    assert all(order.index(x) + 1 >= lds for x in set(b"".join(fz.WORDS[:3]))), "a letter of the three words would lie in LDS"


def test_the_trip_lines_and_the_long_lines():
    r = 1000
    ls = fz.trip_lines(r)
    assert len(ls) == r + 1 and len(set(ls)) <= 8
    one = fz.SETS["one"]
    assert fz.word(*one[:2], ls[0]) == 1 and fz.word(*one[:2], ls[r]) == 0 and fz.distance(fz.WORDS[0], ls[r]) == fz.WORD_KS[0] + 1
    assert 0 < bits(ls, "one")[0] < r
    # limit_lines(): the long lines' matches lie in their last bytes alone
    strs = oracle_strs(lp.limit_ms(), lp.buffer(lp.limit_lines()))
    assert {16000, 64000} <= {len(x) for x in strs} and fz.LONG_TAIL == lp.LIMIT_NEEDLE
    pats, ks = fz.LONG_SET
    w = fz.words(pats, ks, strs)
    for x, word in zip(strs, w):
        if len(x) == 64000:
            assert int(word) & 9 and fz.word(pats, ks, x[:-8]) & 9 == 0, len(x)
    assert all(0 < int(((w >> np.uint64(p)) & np.uint64(1)).sum()) < len(strs) for p in range(4))
