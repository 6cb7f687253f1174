"""Seen sets that count (include/stringsext_amd.h: SX_SEEN_COUNTED, sx_result_seen_counts_device,
sx_result_select_labels_range_device; the kernels of stringsext_amd/csrc/sx_seen_count_dev.hip): how many results held each string,
and how often.  The model is a Python Counter over the strings a scan holds — those of a second Scanner without the flag, or the
oracle's rows for the planted sources —, carried across the calls.  No expected value comes from the code under test.  The sizes are
the smallest at which the kernels can go wrong: counts around a wavefront with seen and new classes alternating inside it, and

    S = CUs x kSeenCountGroupsPerCu x kRowsWaves x 64      records or source words that fill one trip of the count kernels' grid

plus one."""
import collections
import ctypes as C

import numpy as np
import pytest

import refconfig as rc
import result_plant as rp
import stringsext_amd as sx
from test_gpu_distinct_device import flat, strings
from test_gpu_result_strides import constant, scanned, words_of
from test_gpu_seen_device import Stream, entry_bytes
from test_gpu_select_device import check_selection
from test_gpu_select_set_device import Source, code_of

pytestmark = pytest.mark.gpu

M32 = (1 << 32) - 1
RS, FS = sx.SX_SEEN_RESULTS_SHIFT, sx.SX_SEEN_FINDINGS_SHIFT
FIRST, REPEATED, SHIFT = sx.SX_DISTINCT_FIRST, sx.SX_DISTINCT_REPEATED, sx.SX_DISTINCT_COUNT_SHIFT


def word(results, findings):
    return results << RS | findings << FS


def halves(w):
    return w >> RS & M32, w >> FS & M32


class Counts:
    """{key: (results, findings)} carried across the calls; a key is a string under the set's fold (bytes.lower() folds 'A'..'Z' only)"""

    def __init__(self, nocase=False):
        self.key = (lambda s: s.lower()) if nocase else (lambda s: s)
        self.c = {}

    def add(self, k, results, findings):
        r, f = self.c.get(k, (0, 0))
        self.c[k] = (min(M32, r + results), min(M32, f + findings))

    def result(self, strs):
        """one result, or one list: results += 1 per class, findings += its size"""
        for k, n in collections.Counter(self.key(s) for s in strs).items():
            self.add(k, 1, n)

    def words(self, strs):
        return [word(*self.c[self.key(s)]) if self.key(s) in self.c else 0 for s in strs]

    def room(self, extra=0):
        return len(self.c) + extra, sum(entry_bytes(len(k)) for k in self.c) + 64 * extra


def lines(kind, n):
    return [b"%s line number %05d of the buffer" % (kind, k) for k in range(n)]


def buffer_of(ls):
    return b"\n".join(ls) + b"\n" + bytes(4096)


MS2 = rc.missions(encodings=["ascii", "utf-8"], chars_min="10")      # ASCII text under two Missions: every line is found twice
MS1 = rc.missions(encodings=["utf-8"], chars_min="10")


@pytest.fixture(scope="module")
def stream():
    """three small buffers under two Missions whose lines overlap: lines all hold, lines two hold, lines one holds, lines a buffer
    repeats, and lines that differ in case alone"""
    every, ab, bc, a, b, c = lines(b"every", 150), lines(b"ab", 90), lines(b"bc", 70), lines(b"only a", 130), lines(b"only b", 60), lines(b"only c", 80)
    d = [buffer_of(every + ab + a + every[:30] + [b"MiXed Case Line here", b"in a alone: Case"]),
         buffer_of(b + every + ab[::2] + bc + b[:20] + [b"mixed case line here", b"mixed case line here"]),
         buffer_of(bc + c + every[::3] + [b"MIXED CASE LINE HERE", b"in c alone: case"] + every[:10])]
    out = [Source(MS2, x) for x in d]
    yield out
    for s in out:
        s.close()


def fed(stream, ss, model, upto=3):
    """the stream's first buffers through `ss` and the model"""
    for s in stream[:upto]:
        s.res.seen_device(ss).free()
        model.result(strings(s.all_f))


@pytest.mark.parametrize("ignore_case", [False, True])
def test_a_stream_of_three_buffers_into_one_counted_set(stream, ignore_case):
    model, seen = Counts(ignore_case), Stream(ignore_case)
    ss = stream[0].sc.seen_set(2000, 200_000, ignore_case=ignore_case, counted=True)
    try:
        assert ss.counted and ss.counts() == {}
        for k, s in enumerate(stream):
            strs = strings(s.all_f)
            assert min(collections.Counter(strs).values()) >= 2                          # two Missions: every class has two members or more
            lab = s.res.seen_device(ss)
            want_words, want_info = seen.expect(s.all_f)
            assert flat(lab, s.src) == want_words and {f: lab.info[f] for f in want_info} == want_info      # words and info as a plain set's
            lab.free()
            model.result(strs)
            assert ss.counts() == model.c, k
            lab = s.res.seen_counts_device(ss)
            want = model.words(strs)
            assert flat(lab, s.src) == want and all(want)
            sel = s.res.select_range_device(lab, RS, 32, 2, M32)                          # held by two results or more
            kept = [f for f, w in zip(s.all_f, want) if halves(w)[0] >= 2]
            assert bool(kept) == (k > 0)
            if kept:
                check_selection(s.sc, s.src, sel, kept, s.all_f, s.ms, prints=True)
            else:
                assert len(sel) == 0 and sel.device_segments() == []
            sel.free(); lab.free()
        key = model.key
        assert model.c[key(b"every line number 00000 of the buffer")] == (3, 2 * 5)      # 2 + 1 + 2 lines, under two Missions
        assert model.c[key(b"only c line number 00007 of the buffer")] == (1, 2)
        assert (model.c[b"mixed case line here"] == (3, 8)) if ignore_case else (model.c[b"mixed case line here"] == (1, 4) and model.c[b"MiXed Case Line here"] == (1, 2))
        # the counts where another result's findings lie: strings the set does not hold give 0
        other = Source(MS2, buffer_of(lines(b"every", 5) + lines(b"never seen", 400)))
        try:
            lab = other.res.seen_counts_device(ss)
            got, want = flat(lab, other.src), model.words(strings(other.all_f))
            assert got == want and want.count(0) == 800 and len(want) == 810
            lab.free()
        finally:
            other.close()
        ss.reset()
        assert ss.counts() == {} and ss.info()["strings"] == 0
        stream[2].res.seen_device(ss).free()                                             # after a reset the counts begin again
        again = Counts(ignore_case)
        again.result(strings(stream[2].all_f))
        assert ss.counts() == again.c
    finally:
        ss.free()


def entries(blob):
    """the entry area of a blob, entry by entry"""
    n = int.from_bytes(blob[24:32], "little")
    out, at = [], 64
    while at < 64 + n:
        size = entry_bytes(int.from_bytes(blob[at:at + 4], "little"))
        out.append(blob[at:at + size])
        at += size
    return out


def test_a_plain_set_next_to_the_counted_one(stream):
    sc = stream[0].sc
    counted, plain, never = sc.seen_set(2000, 200_000, counted=True), sc.seen_set(2000, 200_000, counted=False), sc.seen_set(2000, 200_000)
    try:
        assert counted.counted and not plain.counted and not never.counted
        for s in stream:
            labs = [s.res.seen_device(x) for x in (counted, plain, never)]
            words = [flat(lab, s.src) for lab in labs]
            assert words[0] == words[1] == words[2] and labs[0].info == labs[1].info == labs[2].info
            for lab in labs:
                lab.free()
            assert counted.info() == plain.info() == never.info()
            assert sorted(counted.strings()) == sorted(plain.strings()) == sorted(never.strings())
        blobs = [x.export() for x in (counted, plain, never)]
        n, nbytes = plain.info()["strings"], plain.info()["bytes"]
        assert [sx.seen_blob_info(b)["version"] for b in blobs] == [2, 1, 1]
        assert [len(b) for b in blobs] == [64 + nbytes + 8 * n, 64 + nbytes, 64 + nbytes]
        assert sorted(entries(blobs[0])) == sorted(entries(blobs[1])) == sorted(entries(blobs[2]))      # (where an entry lies is no part of the contract)
        assert blobs[1][:32] == blobs[2][:32] and blobs[0][12:32] == blobs[1][12:32]
        assert code_of(lambda: plain.counts()) == sx.SX_E_INVALID
        # one wavefront's list: the lanes' entries lie in lane order, so the exports can be compared byte for byte
        few = [b"string %d of a short list" % k for k in range(40)]
        for x in (counted, plain, never):
            x.reset()
            x.add_strings(few)
        blobs = [x.export() for x in (counted, plain, never)]
        assert blobs[1] == blobs[2] and blobs[0][64:64 + len(blobs[1]) - 64] == blobs[1][64:] and blobs[0][12:32] == blobs[1][12:32]
        assert blobs[0][64 + len(blobs[1]) - 64:] == word(1, 1).to_bytes(8, "little") * len(few)
    finally:
        counted.free(); plain.free(); never.free()


def test_the_add_phase_when_nothing_is_new(stream):
    s = stream[1]
    model = Counts()
    ss = s.sc.seen_set(*model_room(s), counted=True)
    try:
        for k in range(2):
            lab = s.res.seen_device(ss)
            assert lab.info["added_strings"] == (0 if k else len(set(strings(s.all_f)))) and lab.info["seen_distinct"] == (lab.info["distinct"] if k else 0)
            lab.free()
            model.result(strings(s.all_f))
            assert ss.counts() == model.c
        assert {r for r, _ in ss.counts().values()} == {2}
        lab = s.res.seen_device(ss, add=False)                                            # lookup-only: the counts stay
        lab.free()
        assert ss.counts() == model.c
    finally:
        ss.free()


def model_room(s, extra=0):
    m = Counts()
    m.result(strings(s.all_f))
    return m.room(extra)


def test_what_does_not_fit_leaves_counts_strings_and_export(stream):
    s1, s2 = stream[0], stream[1]
    both = Counts()
    both.result(strings(s1.all_f)); both.result(strings(s2.all_f))
    cap_s, cap_b = both.room()
    for short_s, short_b in ((1, 0), (0, 8)):
        ss, model = s1.sc.seen_set(cap_s - short_s, cap_b - short_b, counted=True), Counts()
        try:
            fed(stream, ss, model, upto=1)
            before = ss.export(), ss.counts(), ss.info()
            assert code_of(lambda: s2.res.seen_device(ss)) == sx.SX_E_NOMEM
            assert (ss.export(), ss.counts(), ss.info()) == before and ss.counts() == model.c
            new = sorted(set(strings(s2.all_f)))
            assert code_of(lambda: ss.add_strings(new)) == sx.SX_E_NOMEM
            assert (ss.export(), ss.counts(), ss.info()) == before
        finally:
            ss.free()
    ss, model = s1.sc.seen_set(cap_s, cap_b, counted=True), Counts()                       # exactly enough: succeeds
    try:
        fed(stream, ss, model, upto=2)
        assert ss.counts() == model.c == both.c and ss.info()["strings"] == cap_s and ss.info()["bytes"] == cap_b
    finally:
        ss.free()


def test_merge_grow_save_and_load(stream, tmp_path, monkeypatch):
    sc = stream[0].sc
    a, b, plain = sc.seen_set(2000, 200_000, counted=True), sc.seen_set(2000, 200_000, counted=True), sc.seen_set(2000, 200_000)
    ma, mb, mp = Counts(), Counts(), Counts()
    monkeypatch.setenv("SX_SEEN_TAG_BITS", "0")
    other = sx.Scanner(MS1, device=0)
    monkeypatch.delenv("SX_SEEN_TAG_BITS")
    loaded = []
    try:
        fed(stream[:2], a, ma); fed(stream[1:], b, mb); fed(stream[2:], plain, mp)
        before = a.counts()
        a.merge(b, add=False)                                                             # lookup-only
        assert a.counts() == before == ma.c
        info = a.merge(b)                                                                 # counted + counted: the counts add
        assert info["source_strings"] == len(mb.c) and info["already_held"] == len(set(ma.c) & set(mb.c))
        for k, (r, f) in mb.c.items():
            ma.add(k, r, f)
        assert a.counts() == ma.c and b.counts() == mb.c
        a.merge(plain)                                                                    # plain -> counted: (1, 1) per string
        for k in mp.c:
            ma.add(k, 1, 1)
        assert a.counts() == ma.c
        held = set(plain.strings())
        plain.merge(a)                                                                    # counted -> plain: a plain merge
        assert set(plain.strings()) == held | set(ma.c) and not plain.counted and sx.seen_blob_info(plain.export())["version"] == 1
        log2 = a.info()["table_log2"]
        a.grow(5000, 300_000)                                                             # grow: every count under another table_log2
        assert a.info()["table_log2"] > log2 and a.counted and a.counts() == ma.c
        path = str(tmp_path / "counted.sxseen")
        a.save(path)
        assert sx.seen_blob_info(path) == dict(strings=len(ma.c), bytes=a.info()["bytes"], nocase=0, version=2)
        loaded.append(other.seen_set_from(path))                                          # another context, other tag bits
        assert loaded[0].info()["tag_bits"] == 0 and a.info()["tag_bits"] == 24 and loaded[0].counted and loaded[0].counts() == ma.c
        loaded.append(other.seen_set_from(plain.export()))                                # a version-1 blob loads as a plain set
        assert not loaded[1].counted and set(loaded[1].strings()) == set(plain.strings())
        s = stream[0]
        lab, lab2 = s.res.seen_counts_device(a), s.res.seen_counts_device(loaded[0])
        assert flat(lab, s.src) == flat(lab2, s.src) == ma.words(strings(s.all_f))
        lab.free(); lab2.free()
        blob = a.export()
        for bad in (blob[:-8], blob + bytes(8), blob[:-1] + bytes([blob[-1] ^ 1])):
            out = C.c_void_p(0xDEAD0)
            assert sx.lib().sx_seen_set_import(other.h, bad, len(bad), 0, 0, C.byref(out)) == sx.SX_E_INVALID and out.value is None
    finally:
        for x in [a, b, plain] + loaded:
            x.free()
        other.close()


def test_add_strings_with_duplicates_is_one_result(stream):
    sc = stream[0].sc
    for ignore_case in (False, True):
        ss, model = sc.seen_set(100, 10_000, ignore_case=ignore_case, counted=True), Counts(ignore_case)
        try:
            asked = [b"ABC", b"abc", b"", b"Abc", b"seven77", b"", b"abc", b"x" * 300, b"abc", b""]
            info = ss.add_strings(asked)
            model.result(asked)
            assert info["source_strings"] == len(model.c) and ss.counts() == model.c
            assert model.c[b"abc"] == ((1, 5) if ignore_case else (1, 3)) and model.c[b""] == (1, 3)
            before = ss.counts()
            ss.add_strings(asked, add=False)                                              # lookup-only
            assert ss.contains([b"abc", b"nope"]) == [True, False] and ss.counts() == before
            ss.add_strings(asked[:4])
            model.result(asked[:4])
            assert ss.counts() == model.c
        finally:
            ss.free()


def trip_records():
    """S: the records (or source words) that fill one trip of the count kernels' grid"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count      # hipDeviceAttributeMultiprocessorCount: what rows_grid asks
    assert cus > 0 and constant("kSelectRecs") == 64
    return cus * constant("kSeenCountGroupsPerCu") * constant("kRowsWaves") * 64


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_counts_around_a_wavefront_with_seen_and_new_alternating(n):
    """(a result of n findings: the selection of n planted lines out of a buffer that is large enough to stay on the device)"""
    ls = lines(b"edge", n)
    s = Source(MS1, buffer_of(lines(b"filler", 400) + ls))
    res = s.res.select_device(b"edge line")
    all_f = [f for f in s.all_f if b"edge line" in f["s"].encode("utf-8")]
    src = res.device_segments()
    ss, dst = s.sc.seen_set(2 * n + 2, 128 * n + 128, counted=True), s.sc.seen_set(4 * n + 4, 128 * n + 128, counted=True)
    model, md = Counts(), Counts()
    try:
        strs = strings(all_f)
        assert sorted(strs) == sorted(ls) and len(res) == n
        ss.add_strings(strs[::2])                                                         # every other record's string is held: seen, new, seen, ...
        model.result(strs[::2])
        lab = res.seen_device(ss)                                                         # seen_count_kernel
        assert lab.info["seen_distinct"] == len(strs[::2]) and lab.info["added_strings"] == n - len(strs[::2])
        lab.free()
        model.result(strs)
        assert ss.counts() == model.c
        lab = res.seen_counts_device(ss)                                                  # seen_counts_lookup_kernel
        assert flat(lab, src) == model.words(strs)
        lab.free()
        dst.add_strings(strs[1::2] + [b"in the destination alone"])
        md.result(strs[1::2] + [b"in the destination alone"])
        dst.merge(ss)                                                                     # seen_merge_count_kernel, a table as the source
        for k, (r, f) in model.c.items():
            md.add(k, r, f)
        assert dst.counts() == md.c
        dst.add_strings(strs + strs[:n // 2])                                             # ... and a list as the source, with multiplicities
        md.result(strs + strs[:n // 2])
        assert dst.counts() == md.c
        lab = res.seen_counts_device(dst)
        sel = res.select_range_device(lab, FS, 32, md.c[strs[0]][1], M32)                 # label_range_pick_kernel
        want = [f for f, w in zip(all_f, md.words(strs)) if halves(w)[1] >= md.c[strs[0]][1]]
        assert 0 < len(want) <= n
        check_selection(s.sc, src, sel, want, all_f, s.ms, prints=False)
        sel.free(); lab.free()
    finally:
        ss.free(); dst.free(); res.free(); s.close()


def test_one_record_more_than_a_trip_of_the_count_kernels():
    S = trip_records()
    s = scanned("one_over_count", rp.ms1(), rp.prefix(S + 1), S + 1, env=(("SX_WAVE_REPLAY", "1"),))
    strs = list(s.rows.strs)
    classes = collections.Counter(strs)
    distinct = list(classes)
    ss = s.sc.seen_set(len(distinct) + 1, sum(entry_bytes(len(k)) for k in distinct) + 64, counted=True)
    try:
        ss.add_strings(distinct[::2])                                                     # seen and new alternate; the list's count pass
        lab = s.res.seen_device(ss)                                                       # S + 1 records: trip 2 of seen_count_kernel holds one
        assert lab.info["distinct"] == len(distinct) and lab.info["seen_distinct"] == len(distinct[::2])
        lab.free()
        held = set(distinct[::2])
        want = {k: (2 if k in held else 1, n + (1 if k in held else 0)) for k, n in classes.items()}
        assert ss.counts() == want
        lab = s.res.seen_counts_device(ss)                                                # ... and of seen_counts_lookup_kernel
        got = words_of(s.sc, lab, s.res)
        lab.free()
        word_of = {k: word(*v) for k, v in want.items()}
        assert np.array_equal(got, np.array([word_of[x] for x in strs], dtype=np.uint64))
        if len(distinct) > S:                                                             # a list of more than a trip: seen_merge_count_kernel strides
            ss.add_strings(distinct)
            assert ss.counts() == {k: (r + 1, f + 1) for k, (r, f) in want.items()}
    finally:
        ss.free(); s.close(); s.sc.close()


def test_a_list_of_one_word_more_than_a_trip():
    S = trip_records()
    many = [b"%07x" % (k * 2654435761 & 0xFFFFFFF) + b"%d" % k for k in range(S + 1)]
    sc = sx.Scanner(MS1, device=0)
    ss = sc.seen_set(S + 1, sum(entry_bytes(len(x)) for x in many), counted=True)
    try:
        ss.add_strings(many[::2])
        ss.add_strings(many)                                                              # S + 1 source words: trip 2 holds one
        got = ss.counts()
        assert len(got) == S + 1 and got[many[-1]] == ((2, 2) if S % 2 == 0 else (1, 1))
        assert got == {x: ((2, 2) if k % 2 == 0 else (1, 1)) for k, x in enumerate(many)}
    finally:
        ss.free(); sc.close()


def test_range_selection_on_distinct_words(stream):
    s = stream[0]
    lab = s.res.distinct_device()
    try:
        words = flat(lab, s.src)
        by_mask = s.res.select_device(lab, all=REPEATED)
        got_mask = by_mask.findings()
        by_mask.free()
        by_range = s.res.select_range_device(lab, SHIFT, 32, 2, M32)                      # the strings that occur twice or more
        want = [f for f, w in zip(s.all_f, words) if w >> SHIFT >= 2]
        assert by_range.findings() == got_mask == want
        by_range.free()
        sizes = collections.Counter(strings(s.all_f))
        for shift, bits, lo, hi in ((SHIFT, 32, 3, M32), (SHIFT, 32, 4, 4), (SHIFT, 32, 5, 4), (0, 1, 1, 1), (0, 64, 0, (1 << 64) - 1), (1, 63, 1 << 31, 3 << 31)):
            sel = s.res.select_range_device(lab, shift, bits, lo, hi)
            want = [f for f, w in zip(s.all_f, words) if lo <= (w >> shift & (1 << bits) - 1) <= hi]
            if want:
                check_selection(s.sc, s.src, sel, want, s.all_f, s.ms, prints=False)
            else:
                assert len(sel) == 0
            sel.free()
        assert max(sizes.values()) >= 4
    finally:
        lab.free()


def test_refusals(stream):
    s, s2 = stream[0], stream[1]
    L = sx.lib()
    counted, plain = s.sc.seen_set(2000, 200_000, counted=True), s.sc.seen_set(2000, 200_000)
    lab = s.res.distinct_device()
    try:
        for name in ("sx_result_seen_counts_device", "sx_result_select_labels_range_device"):
            assert name in sx.EXPORTS and getattr(L, name)
        assert L.sx_abi_version() == 4 == sx.ABI_VERSION
        assert sx.SX_SEEN_COUNTED not in (sx.SX_SELECT_ASCII_NOCASE, sx.SX_SELECT_INVERT, sx.SX_SEEN_LOOKUP_ONLY)
        out = C.c_void_p(0xDEAD0)
        # the counts of a plain set
        assert L.sx_result_seen_counts_device(s.sc.h, s.res.h, plain.h, C.byref(out)) == sx.SX_E_INVALID and out.value is None
        assert "SX_SEEN_COUNTED" in L.sx_last_error(s.sc.h).decode()
        # NULL arguments
        for args in ((None, s.res.h, counted.h), (s.sc.h, None, counted.h), (s.sc.h, s.res.h, None)):
            out = C.c_void_p(0xDEAD0)
            assert L.sx_result_seen_counts_device(*args, C.byref(out)) == sx.SX_E_INVALID and out.value is None
        assert L.sx_result_seen_counts_device(s.sc.h, s.res.h, counted.h, None) == sx.SX_E_INVALID
        for args in ((None, s.res.h, lab.h), (s.sc.h, None, lab.h), (s.sc.h, s.res.h, None)):
            out = C.c_void_p(0xDEAD0)
            assert L.sx_result_select_labels_range_device(*args, 0, 1, 0, 1, C.byref(out)) == sx.SX_E_INVALID and out.value is None
        assert L.sx_result_select_labels_range_device(s.sc.h, s.res.h, lab.h, 0, 1, 0, 1, None) == sx.SX_E_INVALID
        # a bad field
        for shift, bits in ((0, 0), (0, 65), (1, 64), (64, 1), (33, 32), (0xFFFFFFFF, 2), (63, 2)):
            out = C.c_void_p(0xDEAD0)
            assert L.sx_result_select_labels_range_device(s.sc.h, s.res.h, lab.h, shift, bits, 0, 1, C.byref(out)) == sx.SX_E_INVALID and out.value is None, (shift, bits)
        # labels made from another result
        out = C.c_void_p(0xDEAD0)
        assert L.sx_result_select_labels_range_device(s2.sc.h, s2.res.h, lab.h, 0, 1, 1, 1, C.byref(out)) == sx.SX_E_INVALID and out.value is None
        assert "not made from this result" in L.sx_last_error(s2.sc.h).decode()
        # a host-only context
        host = sx.Scanner([rc.mission()], device=sx.SX_HOST_ONLY)
        try:
            out = C.c_void_p(0xDEAD0)
            assert L.sx_result_seen_counts_device(host.h, s.res.h, counted.h, C.byref(out)) == sx.SX_E_STATE and out.value is None
            out = C.c_void_p(0xDEAD0)
            assert L.sx_result_select_labels_range_device(host.h, s.res.h, lab.h, 0, 1, 1, 1, C.byref(out)) == sx.SX_E_STATE and out.value is None
            out = C.c_void_p(0xDEAD0)
            assert L.sx_seen_set_create(host.h, 10, 100, sx.SX_SEEN_COUNTED, C.byref(out)) == sx.SX_E_STATE and out.value is None
        finally:
            host.close()
        # the flags: what was refused stays refused
        for flags in (sx.SX_SELECT_INVERT, sx.SX_SEEN_COUNTED | sx.SX_SELECT_INVERT, sx.SX_SEEN_LOOKUP_ONLY, 1 << 31):
            out = C.c_void_p(0xDEAD0)
            assert L.sx_seen_set_create(s.sc.h, 10, 100, flags, C.byref(out)) == sx.SX_E_INVALID and out.value is None
        for flags in (1, 2, sx.SX_SEEN_COUNTED, 1 << 31):
            out = C.c_void_p(0xDEAD0)
            assert L.sx_result_seen_device(s.sc.h, s.res.h, counted.h, flags, C.byref(out), None) == sx.SX_E_INVALID and out.value is None
        # the calls themselves work, and age no selection
        words = s.res.seen_counts_device(counted)
        assert set(flat(words, s.src)) == {0}                                             # an empty set holds nothing
        words.free()
    finally:
        lab.free(); counted.free(); plain.free()
