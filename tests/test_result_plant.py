"""tests/result_plant.py against the oracle, at a small size: conditions on the INPUTS of tests/test_gpu_result_strides.py and
tests/test_gpu_result_edges.py, which hold for the reference alone — no product code runs here."""
import collections

import pytest

import result_plant as rp

N = 6000      # lines: several 4096-byte windows of the reference's scan, and every kind of line the plant has


@pytest.fixture(scope="module")
def lines():
    return rp.lines(N)


def test_lines_are_4_to_60_printable_bytes_of_every_length_modulo_16(lines):
    assert all(4 <= len(x) <= 60 and all(0x20 <= b < 0x7F for b in x) for x in lines)
    assert {len(x) % 16 for x in lines} == set(range(16))
    assert {len(x) for x in lines} >= {4, 60}
    assert rp.lines(100) == lines[:100] and rp.buffer(N) == b"\n".join(lines) + b"\n"      # a prefix of the same lines, whatever was asked first


def test_with_one_mission_line_k_is_finding_k(lines):
    e = rp.expected(rp.ms1(), rp.buffer(N))
    assert e.strs == lines
    assert all(r[2] == b"" and r[1][1:] == b" " for r in e.rows)                # no Mission label, and no finding continues another
    assert list(e.position) == sorted(e.position) and len(set(e.position.tolist())) > N // 10 and set(e.precision.tolist()) == {0, 1, 2}
    assert [e.uniq[i] for i in e.inv] == e.strs and e.uniq == list(dict.fromkeys(lines))


def test_with_two_missions_every_line_is_found_once_by_each_in_line_order(lines):
    e = rp.expected(rp.ms2(), rp.buffer(N))
    assert e.n == 2 * N and {r[2] for r in e.rows} == {b"(a ascii)", b"(b UTF-8)"}
    for m in (0, 1):
        assert [s for s, x in zip(e.strs, e.mission.tolist()) if x == m] == lines
    # the merged order is the reference's, by window and then by Mission: both Missions alternate in stretches, never line by line only
    assert e.mission.tolist() != sorted(e.mission.tolist()) and list(e.position) == sorted(e.position)


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513])
def test_a_prefix_has_exactly_k_findings_and_ends_with_the_sentinel(k, lines):
    data = rp.prefix(k)
    assert data == b"".join(x + b"\n" for x in lines[:k - 1]) + rp.SENTINEL + b"\n"
    e = rp.expected(rp.ms1(), data)
    assert e.n == k and e.strs == lines[:k - 1] + [rp.SENTINEL]
    e2 = rp.expected(rp.ms2(), data)
    assert e2.n == 2 * k and e2.strs[-1] == rp.SENTINEL


def test_the_sentinel_matches_every_pattern_and_repeats_line_0_and_line_1_under_the_fold(lines):
    assert lines[0] == rp.SENTINEL and lines[1] != rp.SENTINEL and lines[1].lower() == rp.SENTINEL.lower()
    assert 4 <= len(rp.SENTINEL) <= 60
    for name, pred in rp.predicates().items():
        assert pred(rp.SENTINEL), name
    for r in rp.LABELS + rp.REGEXES + rp.EXTRACTS:
        assert rp.to_python(r).search(rp.SENTINEL), r
    occ = rp.occurrences([rp.SENTINEL], rp.keyword_list())
    assert any(occ) and rp.occurrences([rp.SENTINEL], [b"77", b"777", rp.HOT_SHORT]) == [{0: 4}, {0: 3}, {0: 1}]      # overlapping places count


@pytest.mark.parametrize("n", [600, N])
def test_every_predicate_selects_5_to_60_percent(n):
    e = rp.expected(rp.ms1(), rp.buffer(n))
    for name, pred in rp.predicates().items():
        share = e.mask(pred).mean()
        assert 0.05 <= share <= 0.60, (name, share)
    kw = rp.keyword_list()
    occ = rp.occurrences(e.uniq, kw)
    assert 1900 <= len(kw) <= 2100 and len(set(kw)) == len(kw) and all(len(p) >= 4 for p in kw)
    assert (24 if n == N else 5) <= sum(1 for d in occ if d) <= 60 and 0.05 <= rp.held_by_any(e, occ).mean() <= 0.60
    # the prefix token stands only at the beginning of a line, the suffix token only at its end; a kind stands at the beginning or
    # behind the prefix token, so that `^` and `$` decide
    assert all(x.find(b"-> ") <= 0 and x.find(b" ;;") in (-1, len(x) - 3) for x in e.uniq)
    assert any(x.find(b"mmap") == 0 for x in e.uniq) and any(x.find(b"mmap") > 0 for x in e.uniq)


def test_occurrences_is_the_rule_of_the_header(lines):
    """hits of a keyword in a string: the places o with s[o:o + len(p)] == p"""
    kw = rp.tally_list()
    uniq = list(dict.fromkeys(lines))[:400]
    occ = rp.occurrences(uniq, kw)
    assert len(set(kw)) == len(kw) > 4096 + 100
    for k in list(range(0, len(kw), 97)) + [kw.index(p) for p in (rp.HOT_SHORT, rp.HOT_LONG, b"77", b"777")]:
        want = {u: c for u, c in ((u, sum(s.startswith(kw[k], o) for o in range(len(s)))) for u, s in enumerate(uniq)) if c}
        assert occ[k] == want, kw[k]
    assert len(occ[kw.index(rp.HOT_SHORT)]) > 300 and occ[kw.index(rp.HOT_LONG)] == {uniq.index(rp.DOMINANT): 1}


def test_the_mix_of_classes_the_dominant_line_and_the_fold(lines):
    size = collections.Counter(lines)
    by_size = collections.Counter(min(c, 3) for c in size.values())
    assert all(by_size[c] >= N // 100 for c in (1, 2, 3)), by_size
    repeats = N - len(size)
    assert 0.55 <= repeats / N <= 0.75                                            # about two lines of three repeat an earlier one
    assert size[rp.DOMINANT] == max(size.values()) >= N // 30
    at = [k for k, x in enumerate(lines) if x == rp.DOMINANT]
    runs = collections.Counter()
    run = 1
    for a, b in zip(at, at[1:] + [-1]):
        if b == a + 1:
            run += 1
        else:
            runs[run] += 1
            run = 1
    assert runs[1] > 10 and runs[3] + runs[4] > 10 and max(runs) >= 70            # scattered, in runs of neighbours, and a run longer than a wavefront
    # the fold joins classes that the plain comparison keeps apart, and only some
    folded = collections.Counter(x.lower() for x in lines)
    assert len(folded) < len(size) - N // 100 and len(folded) > len(size) // 2
    plain, _, _, _ = rp.distinct_model(lines, 1, 2, 32)
    nocase, info, _, _ = rp.distinct_model(lines, 1, 2, 32, nocase=True)
    assert info == dict(findings=N, distinct=len(folded), repeated=sum(1 for c in folded.values() if c > 1))
    assert (plain != nocase).sum() > N // 100


def test_the_distinct_model_is_the_dict_rule(lines):
    """tests/test_gpu_distinct_device.py's py_words, which is the rule, on the same strings"""
    for nocase in (False, True):
        keys = [x.lower() if nocase else x for x in lines]
        size = collections.Counter(keys)
        seen, want = set(), []
        for k in keys:
            want.append((1 if k not in seen else 0) | (2 if size[k] > 1 else 0) | size[k] << 32)
            seen.add(k)
        words, info, classes, inv = rp.distinct_model(lines, 1, 2, 32, nocase=nocase)
        assert words.tolist() == want and info["distinct"] == len(size) and classes == list(dict.fromkeys(keys))
        assert [classes[i] for i in inv] == keys


def test_a_token_on_exactly_k_lines():
    for n, k in ((600, 1), (600, 64), (2000, 512), (2000, 513)):
        e = rp.expected(rp.ms1(), rp.with_token(n, k))
        assert e.n == n and sum(1 for s in e.strs if b"{pick}" in s) == k and all(4 <= len(s) <= 60 for s in e.strs)
        assert not any(b"{pick}" in p or p in b"{pick}" for p in rp.keyword_list() + rp.tally_list() + rp.SIXTEEN)      # (the token is no keyword)
