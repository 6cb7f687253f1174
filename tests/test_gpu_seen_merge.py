"""Seen sets that outlive a call (include/stringsext_amd.h: sx_seen_set_merge, _grow, _export, _import, _add_strings; the kernels of
stringsext_amd/csrc/sx_seen_merge_dev.hip): merged, grown, saved and loaded, and fed from lists of strings.  The model is Python sets
of (folded) byte strings; what a scan holds comes from a second Scanner without the flag.  No expected value comes from the code under
test.  Sets are filled by add_strings and, in every test, by a real seen_device call on a small scan.  The sizes are the smallest at
which the kernels can go wrong: word counts around a wavefront, and

    S = CUs x kSeenMergeGroupsPerCu x kRowsWaves x 64      source words that fill one trip of the mark kernel's grid

plus one, and a source table that is mostly empty and has 2 S x kSeenMergeAddChunks slots or more: two trips of the add kernel, whose
wavefronts take kSeenMergeAddChunks chunks of 64 words per trip."""
import ctypes as C

import pytest

import refconfig as rc
import stringsext_amd as sx
from test_gpu_distinct_device import flat, strings
from test_gpu_result_strides import constant
from test_gpu_seen_device import SEEN, Stream, entry_bytes
from test_gpu_select_set_device import Source, code_of

pytestmark = pytest.mark.gpu


def lines(kind, n):
    return [b"%s line number %05d of the buffer" % (kind, k) for k in range(n)]


@pytest.fixture(scope="module")
def scans():
    """two small buffers of one Mission whose findings overlap: lines both hold, lines only one holds, and lines a buffer repeats"""
    ms = rc.missions(encodings=["utf-8"], chars_min="10")
    both, one, two = lines(b"shared", 300), lines(b"first", 200), lines(b"second", 250)
    d1 = b"\n".join(both + one + both[:40] + [b"MiXed Case Line"]) + b"\n" + bytes(4096)
    d2 = b"\n".join(two + both + two[:30] + [b"mixed case line"]) + b"\n" + bytes(4096)
    s1, s2 = Source(ms, d1), Source(ms, d2)
    yield s1, s2
    s1.close(); s2.close()


def held_of(source, nocase=False):
    return {s.lower() if nocase else s for s in strings(source.all_f)}


def size_of(strs):
    return dict(strings=len(strs), bytes=sum(entry_bytes(len(s)) for s in strs))


def counts(ss):
    i = ss.info()
    return dict(strings=i["strings"], bytes=i["bytes"])


def want_info(held, src, add=True):
    new = src - held
    return dict(source_strings=len(src), already_held=len(src & held), added_strings=len(new) if add else 0, added_bytes=sum(entry_bytes(len(s)) for s in new) if add else 0)


def lookup_words(source, ss):
    """the words of a lookup-only seen_device call over the source's result"""
    lab = source.res.seen_device(ss, add=False)
    words = flat(lab, source.src)
    lab.free()
    return words


def model_words(source, held, nocase=False):
    m = Stream(nocase)
    m.held = set(held)
    return m.expect(source.all_f, add=False)[0]


def test_merge_two_sets_with_an_overlap(scans):
    s1, s2 = scans
    a, b = held_of(s1), held_of(s2)
    assert len(a & b) > 100 and len(a - b) > 100 and len(b - a) > 100                     # an overlap, and a remainder on either side
    dst, src = s1.sc.seen_set(len(a | b) + 5, size_of(a | b)["bytes"] + 100), s1.sc.seen_set(len(b), size_of(b)["bytes"])
    try:
        s1.res.seen_device(dst).free()                                                    # filled by a scan's result
        assert src.add_strings(sorted(b)) == want_info(set(), b)                          # filled from a list
        assert counts(dst) == size_of(a) and counts(src) == size_of(b) and set(dst.strings()) == a and set(src.strings()) == b
        before, before_src = dst.export(), src.export()
        assert dst.merge(src, add=False) == want_info(a, b, add=False)                    # lookup-only: the intersection, nothing changed
        assert dst.export() == before and src.export() == before_src
        assert dst.merge(src) == want_info(a, b)
        assert src.export() == before_src                                                 # the source is only read
        got = dst.strings()
        assert len(got) == len(a | b) and set(got) == a | b and counts(dst) == size_of(a | b)
        assert dst.export()[64:len(before)] == before[64:]                      # what it held lies where it lay
        assert dst.merge(src) == want_info(a | b, b)                                      # again: all held
        for s in (s1, s2):
            words = lookup_words(s, dst)
            assert words == model_words(s, a | b) and all(w & SEEN for w in words)
        words = lookup_words(s1, src)
        assert words == model_words(s1, b) and any(w & SEEN for w in words) and not all(w & SEEN for w in words)
        # refusals: a set into itself, flags, a freed set; what is new does not fit: the set is as it was, and the message names the sums
        assert code_of(lambda: dst.merge(dst)) == sx.SX_E_INVALID
        assert sx.lib().sx_seen_set_merge(s1.sc.h, dst.h, src.h, 1, None) == sx.SX_E_INVALID
        small = s1.sc.seen_set(len(a | b) - 1, size_of(a | b)["bytes"])
        try:
            s1.res.seen_device(small).free()
            before = small.export()
            assert code_of(lambda: small.merge(src)) == sx.SX_E_NOMEM
            text = sx.lib().sx_last_error(s1.sc.h).decode()
            assert "%d + %d strings of %d" % (len(a), len(b - a), len(a | b) - 1) in text and "%d + %d bytes of %d" % (
                size_of(a)["bytes"], size_of(b - a)["bytes"], size_of(a | b)["bytes"]) in text, text
            assert small.export() == before and small.merge(src, add=False) == want_info(a, b, add=False)
        finally:
            small.free()
    finally:
        dst.free(); src.free()


def test_grow_keeps_the_handle_and_the_strings(scans):
    s1, _ = scans
    a = held_of(s1)
    cap = size_of(a)
    ss = s1.sc.seen_set(cap["strings"], cap["bytes"] + 64)                                # filled to exactly capacity_strings
    try:
        s1.res.seen_device(ss).free()
        info, handle, before = ss.info(), ss.h.value, ss.export()
        assert info["strings"] == info["capacity_strings"] == len(a)
        assert code_of(lambda: ss.add_strings([b"one more new string"])) == sx.SX_E_NOMEM
        assert "sx_seen_set_grow" in sx.lib().sx_last_error(s1.sc.h).decode()
        assert ss.export() == before and ss.info() == info
        assert code_of(lambda: ss.grow(len(a) - 1, cap["bytes"] + 64)) == sx.SX_E_INVALID     # less than it holds: refused, unchanged
        assert code_of(lambda: ss.grow(len(a), cap["bytes"] - 8)) == sx.SX_E_INVALID
        assert code_of(lambda: ss.grow(0, cap["bytes"])) == sx.SX_E_INVALID
        assert ss.export() == before and ss.info() == info and ss.h.value == handle
        ss.grow(2 * len(a), 2 * cap["bytes"] + 128)
        grown = ss.info()
        assert ss.h.value == handle and grown["table_log2"] == info["table_log2"] + 1 and grown["tag_bits"] == info["tag_bits"]
        assert (grown["strings"], grown["bytes"], grown["capacity_strings"], grown["capacity_bytes"]) == (len(a), cap["bytes"], 2 * len(a), 2 * cap["bytes"] + 128)
        assert set(ss.strings()) == a and len(ss.strings()) == len(a)
        assert ss.add_strings([b"one more new string"]) == want_info(a, {b"one more new string"})      # the same call succeeds
        words = lookup_words(s1, ss)
        assert words == model_words(s1, a) and all(w & SEEN for w in words)               # every earlier string is still seen
        assert ss.contains(sorted(a)) == [True] * len(a)
        ss.grow(len(a) + 1, cap["bytes"] + entry_bytes(19))                               # smaller again, to exactly what it holds
        shrunk = ss.info()
        assert (shrunk["strings"], shrunk["bytes"]) == (shrunk["capacity_strings"], shrunk["capacity_bytes"]) == (len(a) + 1, cap["bytes"] + entry_bytes(19))
        assert set(ss.strings()) == a | {b"one more new string"} and lookup_words(s1, ss) == words
    finally:
        ss.free()


def test_save_and_load_under_other_tag_bits_and_another_table(scans, tmp_path, monkeypatch):
    s1, s2 = scans
    a = held_of(s1)
    ss = s1.sc.seen_set(len(a) + 10, size_of(a)["bytes"] + 1000)
    monkeypatch.setenv("SX_SEEN_TAG_BITS", "0")
    other = sx.Scanner(s1.ms, device=0)
    monkeypatch.delenv("SX_SEEN_TAG_BITS")
    loaded = None
    try:
        s1.res.seen_device(ss).free()
        path = str(tmp_path / "baseline.sxseen")
        ss.save(path)
        blob = open(path, "rb").read()
        assert blob == ss.export() and sx.seen_blob_info(path) == dict(strings=len(a), bytes=size_of(a)["bytes"], nocase=0, version=1)
        loaded = other.seen_set_from(path, capacity_strings=8 * len(a))
        i, j = ss.info(), loaded.info()
        assert j["tag_bits"] == 0 and i["tag_bits"] == 24 and j["table_log2"] > i["table_log2"] and j["capacity_bytes"] == size_of(a)["bytes"]
        assert (j["strings"], j["bytes"], j["nocase"]) == (len(a), size_of(a)["bytes"], 0)
        assert set(loaded.strings()) == a == set(ss.strings()) and len(loaded.strings()) == len(a)
        for s in (s1, s2):
            words = lookup_words(s, loaded)
            assert words == lookup_words(s, ss) == model_words(s, a)
        assert any(w & SEEN for w in lookup_words(s2, loaded)) and not all(w & SEEN for w in lookup_words(s2, loaded))
        exact = other.seen_set_from(blob)                                                 # capacities of 0: what the blob holds
        k = exact.info()
        assert (k["strings"], k["bytes"]) == (k["capacity_strings"], k["capacity_bytes"]) == (len(a), size_of(a)["bytes"])
        exact.free()
        # a capacity below what the blob holds, and corrupted files: SX_E_INVALID and no handle
        out = C.c_void_p(0xDEAD0)
        assert sx.lib().sx_seen_set_import(other.h, blob, len(blob), len(a) - 1, 0, C.byref(out)) == sx.SX_E_INVALID and out.value is None
        for bad in (blob[:-8], blob[:100] + bytes([blob[100] ^ 1]) + blob[101:], b"SXSEEM" + blob[6:], blob + bytes(8)):
            open(path, "wb").write(bad)
            out = C.c_void_p(0xDEAD0)
            assert sx.lib().sx_seen_set_import(other.h, bad, len(bad), 0, 0, C.byref(out)) == sx.SX_E_INVALID and out.value is None
            assert "import" in sx.lib().sx_last_error(other.h).decode()
            assert code_of(lambda: other.seen_set_from(path)) == sx.SX_E_INVALID
    finally:
        if loaded:
            loaded.free()
        ss.free(); other.close()


def trip_words():
    """S: the source words that fill one trip of the merge kernels' grid"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count      # hipDeviceAttributeMultiprocessorCount: what rows_grid asks
    assert cus > 0 and constant("kSelectRecs") == 64
    return cus * constant("kSeenMergeGroupsPerCu") * constant("kRowsWaves") * 64


ADD_TRIP = constant("kSeenMergeAddChunks") * constant("kSelectRecs")      # the source words of one trip of seen_merge_add_kernel's wavefront: 512


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, ADD_TRIP - 1, ADD_TRIP, ADD_TRIP + 1])
def test_list_sources_around_a_wavefront(scans, n):
    s1, _ = scans
    a = held_of(s1)
    new = [b"list string %d" % k + b"." * (k % 9) for k in range(n)]
    room = max(200, n)                                                    # (an entry of these strings has 40 bytes at most)
    assert max(entry_bytes(len(s)) for s in new) <= 40
    ss = s1.sc.seen_set(len(a) + room, size_of(a)["bytes"] + room * 40)
    try:
        s1.res.seen_device(ss).free()
        held = {new[0], new[n // 2], new[-1]}
        assert ss.add_strings(sorted(held)) == want_info(a, held)
        assert ss.contains(new) == [s in held for s in new]
        assert ss.add_strings(new) == want_info(a | held, set(new))
        assert ss.contains(new + [b"absent"]) == [True] * n + [False]
        assert set(ss.strings()) == a | set(new) and counts(ss) == size_of(a | set(new))
    finally:
        ss.free()


def test_a_list_of_one_trip_plus_one_and_a_mostly_empty_table_as_the_source(scans):
    s1, _ = scans
    a = held_of(s1)
    S = trip_words()
    many = [b"%07x" % (k * 2654435761 & 0xFFFFFFF) + b"%d" % k for k in range(S + 1)]     # S + 1 distinct short strings: trip 2 holds one word
    assert len(set(many)) == S + 1 and not set(many) & a
    chunks = constant("kSeenMergeAddChunks")
    big = s1.sc.seen_set(S * chunks, sum(entry_bytes(len(s)) for s in many) + 64)           # (a table of 2 S x chunks slots or more)
    dst = s1.sc.seen_set(S + 1 + len(a), sum(entry_bytes(len(s)) for s in many) + size_of(a)["bytes"])
    try:
        s1.res.seen_device(dst).free()
        assert big.add_strings(many) == want_info(set(), set(many))
        got = big.contains(many)
        assert got[-1] and all(got)                                                       # the last string: the one word of trip 2
        absent = many[:-1] + [b"planted and absent"]
        got = big.contains(absent)
        assert not got[-1] and all(got[:-1])
        # set -> set: the source's table holds two trips of the add kernel or more, and two thirds of it or more are empty: the skip path, striding
        slots = 1 << big.info()["table_log2"]
        assert slots >= 2 * S * chunks and 3 * (S + 1) <= slots
        assert dst.add_strings(many[::5]) == want_info(a, set(many[::5]))
        held = a | set(many[::5])
        assert dst.merge(big, add=False) == want_info(held, set(many), add=False)
        assert dst.merge(big) == want_info(held, set(many))
        i = dst.info()
        assert (i["strings"], i["bytes"]) == (i["capacity_strings"], i["capacity_bytes"])             # filled to the last byte
        got = dst.strings()
        assert len(got) == len(a) + S + 1 and set(got) == a | set(many)
    finally:
        big.free(); dst.free()


def test_the_fold_belongs_to_the_set(scans):
    s1, _ = scans
    folded, plain = s1.sc.seen_set(2000, 100_000, ignore_case=True), s1.sc.seen_set(2000, 100_000)
    try:
        assert folded.add_strings([b"ABC", b"abc", b"Abc"]) == dict(source_strings=1, already_held=0, added_strings=1, added_bytes=16)
        assert folded.strings() == [b"abc"]
        assert folded.contains([b"aBC", b"x", b"ABC", b"x", b"abcd", b"ab", b"[BC"]) == [True, False, True, False, False, False, False]      # per input string
        assert folded.add_strings([b"ABC", b"New", b"NEW", b"abc"], add=False) == dict(source_strings=2, already_held=1, added_strings=0, added_bytes=0)
        assert plain.add_strings([b"ABC", b"abc", b"Abc", b"ABC"]) == dict(source_strings=3, already_held=0, added_strings=3, added_bytes=48)
        assert plain.contains([b"aBC", b"ABC"]) == [False, True]
        assert code_of(lambda: folded.merge(plain)) == sx.SX_E_INVALID and code_of(lambda: plain.merge(folded)) == sx.SX_E_INVALID
        assert "fold" in sx.lib().sx_last_error(s1.sc.h).decode()
        # a scan's strings into the folding set, saved and loaded: the fold travels with the blob
        s1.res.seen_device(folded).free()
        a = held_of(s1, nocase=True) | {b"abc"}
        assert b"mixed case line" in a and set(folded.strings()) == a
        loaded = s1.sc.seen_set_from(folded.export())
        try:
            assert loaded.info()["nocase"] == 1 and set(loaded.strings()) == a
            assert loaded.contains([b"MIXED case LINE", b"mixed case line", b"Mixed case lime"]) == [True, True, False]
            assert loaded.merge(folded, add=False) == want_info(a, a, add=False)
        finally:
            loaded.free()
    finally:
        folded.free(); plain.free()


def test_contains_against_a_set_filled_by_a_scan(scans):
    s1, s2 = scans
    a, b = held_of(s1), sorted(held_of(s2))
    ss = s1.sc.seen_set(len(a), size_of(a)["bytes"])
    try:
        s1.res.seen_device(ss).free()
        asked = b[::2] + [b"", b"absent", b[0], b[0], b[1] + b"\x00", b[1][:-1]] + sorted(a)[::3] + b[::7] + [bytes(range(256)) * 40]       # duplicates; one longer than a finding can be
        want = [s in a for s in asked]
        assert any(want) and not all(want)
        before = ss.export()
        assert ss.contains(asked) == want
        assert ss.add_strings(asked, add=False) == want_info(a, set(asked), add=False)
        assert ss.export() == before
        assert ss.contains([]) == [] and ss.add_strings([]) == dict(source_strings=0, already_held=0, added_strings=0, added_bytes=0)
    finally:
        ss.free()
