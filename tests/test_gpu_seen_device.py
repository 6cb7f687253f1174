"""sx_result_seen_device and sx_seen_set (include/stringsext_amd.h): strings remembered in HBM from one device-resident result to the
next (stringsext_amd/csrc/sx_seen_dev.hip) — per finding the word of sx_result_distinct_device plus SX_DISTINCT_SEEN, the set's
contents counted, and what sx_result_select_labels_device makes of the words: the stream's sort -u, baseline subtraction,
intersection.  The expected value never comes from the code under test: a second Scanner without the flag scans the same data, and a
Python set carried from buffer to buffer says which strings were held."""
import ctypes as C
import random

import pytest

import refconfig as rc
import stringsext_amd as sx
from test_gpu_distinct_device import flat, py_words, strings
from test_gpu_result_on_device_multi import case
from test_gpu_select_device import check_selection, downloaded, filtered, pointers
from test_gpu_select_set_device import Source, code_of
from test_host_logic import synth

pytestmark = pytest.mark.gpu

FIRST, REPEATED, SEEN, SHIFT = sx.SX_DISTINCT_FIRST, sx.SX_DISTINCT_REPEATED, sx.SX_DISTINCT_SEEN, sx.SX_DISTINCT_COUNT_SHIFT
COUNTED = ("findings", "distinct", "repeated", "seen_findings", "seen_distinct", "added_strings", "added_bytes")


def entry_bytes(n):
    """SX_SEEN_ENTRY_BYTES"""
    return 8 + (n + 7) // 8 * 8


class Stream:
    """the model: a Python set carried across the buffers"""

    def __init__(self, nocase=False):
        self.nocase, self.held = nocase, set()

    def expect(self, findings, add=True):
        """(the words in print order, the counted fields of sx_seen_info); with add the set then holds the strings"""
        words, info = py_words(findings, self.nocase)
        keys = [s.lower() if self.nocase else s for s in strings(findings)]
        words = [w | (SEEN if k in self.held else 0) for w, k in zip(words, keys)]
        classes = list(dict.fromkeys(keys))
        new = [k for k in classes if k not in self.held]
        info.update(seen_findings=sum(k in self.held for k in keys), seen_distinct=len(classes) - len(new),
                    added_strings=len(new) if add else 0, added_bytes=sum(entry_bytes(len(k)) for k in new) if add else 0)
        if add:
            self.held |= set(new)
        return words, info

    def held_info(self):
        return dict(strings=len(self.held), bytes=sum(entry_bytes(len(k)) for k in self.held))


def decided(words):
    """findings that are seen and first, seen and not first, new and repeated, and new singletons: no comparison is empty"""
    kinds = {(bool(w & SEEN), bool(w & FIRST), w >> SHIFT > 1) for w in words}
    assert {(True, True), (True, False)} <= {k[:2] for k in kinds} and (False, True, True) in kinds and (False, True, False) in kinds, kinds


def held(seen_set):
    i = seen_set.info()
    return dict(strings=i["strings"], bytes=i["bytes"])


def check_call(s, seen_set, model, add=True, res=None, all_f=None):
    """one seen_device call over s.res (or `res`, whose findings are all_f) against the model: the words, the info, the set's contents
    counted; returns (the Labels, the words)"""
    res, all_f = res or s.res, s.all_f if all_f is None else all_f
    src = res.device_segments()
    want, want_info = model.expect(all_f, add)
    lab = res.seen_device(seen_set, add=add)
    got = flat(lab, src)
    print({k: lab.info[k] for k in lab.info}, seen_set.info())
    assert got == want, next((i, hex(a), hex(b), all_f[i]["s"]) for i, (a, b) in enumerate(zip(got, want)) if a != b)
    assert {k: lab.info[k] for k in COUNTED} == want_info, (lab.info, want_info)
    assert held(seen_set) == model.held_info(), (seen_set.info(), model.held_info())
    assert pointers(res) == [(x[0], x[1], x[2], x[3], x[4]) for x in src]                  # read, not moved
    return lab, want


@pytest.fixture(scope="module")
def pair():
    """two different buffers of the same four Missions: case "A", then a synth buffer that repeats some of A's lines and brings its own;
    their findings by a Scanner without the flag"""
    ms, data1, _ = case("A")
    lines = data1[:1_400_000].split(b"\n")
    repeated = lines[5:3000:3]
    data2 = b"\n".join(repeated) + b"\n" + synth(random.Random(91), 1_000_000, 1 / 400) + b"\n" + b"\n".join(repeated[:50]) + b"\n" + bytes(4096)
    ref = sx.Scanner(ms, device=0)
    out = dict(ms=ms, data=[data1, data2], f=[])
    for data in out["data"]:
        ref.reset()
        host = ref.scan(data, file_id=1)
        out["f"].append(host.findings())
        host.free()
    ref.close()
    one, two = set(strings(out["f"][0])), set(strings(out["f"][1]))
    assert len(one & two) > 100 and len(two - one) > 10 and len(one - two) > 100            # an overlap, and a remainder on either side
    return out


def sources(pair):
    return [Source(pair["ms"], pair["data"][k], all_f=pair["f"][k]) for k in (0, 1)]


def test_two_different_buffers_through_one_set(pair):
    """(the two buffers' results live in two contexts: the set of the first is accepted by the second, on the same device)"""
    s1, s2 = sources(pair)
    ss = s1.sc.seen_set(200_000, 16 << 20)
    try:
        assert ss.info() == dict(strings=0, bytes=0, capacity_strings=200_000, capacity_bytes=16 << 20, table_log2=19, nocase=0, tag_bits=24)
        model = Stream()
        lab1, w1 = check_call(s1, ss, model)
        assert not any(w & SEEN for w in w1) and lab1.info["added_strings"] == lab1.info["distinct"]
        lab2, w2 = check_call(s2, ss, model)
        decided(w2)
        # the stream's sort -u: every string new to the stream, once
        new = []
        for s, lab, w in ((s1, lab1, w1), (s2, lab2, w2)):
            want = [f for f, x in zip(s.all_f, w) if x & FIRST and not x & SEEN]
            sel = s.res.select_device(lab, any=FIRST, none=SEEN)
            check_selection(s.sc, s.src, sel, want, s.all_f, s.ms, prints=False)
            new += [f["s"] for f in downloaded(s.sc, sel)]
            sel.free()
        assert new == list(dict.fromkeys(f["s"] for f in s1.all_f + s2.all_f))
        # intersection and baseline subtraction partition buffer 2
        both = [f for f, x in zip(s2.all_f, w2) if x & SEEN]
        only = [f for f, x in zip(s2.all_f, w2) if not x & SEEN]
        assert both and only and len(both) + len(only) == len(s2.all_f)
        for masks, want in ((dict(any=SEEN), both), (dict(none=SEEN), only)):
            sel = s2.res.select_device(lab2, **masks)
            check_selection(s2.sc, s2.src, sel, want, s2.all_f, s2.ms, prints=False)
            sel.free()
        # sx_result_distinct_device on the same result: the seen words without bit 2 (its body is shared with the seen call)
        plain = s2.res.distinct_device()
        assert flat(plain, s2.src) == [w & ~SEEN for w in w2]
        assert {k: plain.info[k] for k in plain.info} == {k: lab2.info[k] for k in plain.info}
        plain.free(); lab1.free(); lab2.free()
        # the set outlives the context that made it
        s1.close()
        s1 = None
        lab, w = check_call(s2, ss, model)
        assert all(x & SEEN for x in w) and lab.info["added_strings"] == 0
        lab.free()
    finally:
        ss.free()
        for s in (s1, s2):
            if s:
                s.close()


def test_a_baseline_looked_up_and_nothing_added(pair):
    s1, s2 = sources(pair)
    ss = s2.sc.seen_set(100_000, 8 << 20)
    try:
        model = Stream()
        lab, _ = check_call(s1, ss, model)
        lab.free()
        before = ss.info()
        lab, want = check_call(s2, ss, model, add=False)
        decided(want)
        assert lab.info["added_strings"] == 0 and lab.info["added_bytes"] == 0 and ss.info() == before
        again, _ = check_call(s2, ss, model, add=False)
        assert flat(again, s2.src) == want and again.info == lab.info and ss.info() == before
        again.free(); lab.free()
        ss.reset()
        assert held(ss) == dict(strings=0, bytes=0)
        lab, want = check_call(s2, ss, Stream())
        assert not any(w & SEEN for w in want)
        lab.free()
    finally:
        ss.free(); s1.close(); s2.close()


def test_a_set_that_folds(pair):
    s1, s2 = sources(pair)
    folded_data = pair["data"][1][:200_000].upper()
    ref = sx.Scanner(pair["ms"], device=0)
    host = ref.scan(folded_data, file_id=1)
    f3 = host.findings()
    host.free(); ref.close()
    s3 = Source(pair["ms"], folded_data, all_f=f3)
    ss, plain = s1.sc.seen_set(200_000, 16 << 20, ignore_case=True), s1.sc.seen_set(200_000, 16 << 20)
    try:
        assert ss.info()["nocase"] == 1 and plain.info()["nocase"] == 0
        model, model_plain = Stream(nocase=True), Stream()
        for s in (s1, s2):
            lab, want = check_call(s, ss, model)
            lab.free()
            lab, _ = check_call(s, plain, model_plain)
            lab.free()
        decided(want)
        lab, want = check_call(s3, ss, model)                       # buffer 2's beginning in capitals: the folding set has seen it
        lab_plain, want_plain = check_call(s3, plain, model_plain)
        assert sum(1 for w in want if w & SEEN) > sum(1 for w in want_plain if w & SEEN) + 100
        lab.free(); lab_plain.free()
    finally:
        ss.free(); plain.free()
        for s in (s1, s2, s3):
            s.close()


def test_without_tags_and_filled_to_the_last_string(pair, monkeypatch):
    """SX_SEEN_TAG_BITS=0: every occupied slot on a probe's way is compared byte for byte; the capacity is exactly what the two buffers
    hold, so the table — the smallest the entry point makes — ends at a load of 1/2 or a little less and the set 100 % full"""
    full = Stream()
    for f in pair["f"]:
        full.expect(f)
    cap = full.held_info()
    monkeypatch.setenv("SX_SEEN_TAG_BITS", "0")
    s1, s2 = sources(pair)
    monkeypatch.delenv("SX_SEEN_TAG_BITS")                           # a context keeps the switch it was created under
    ss = s1.sc.seen_set(cap["strings"], cap["bytes"])
    try:
        info = ss.info()
        assert info["tag_bits"] == 0 and info["table_log2"] == next(p for p in range(1, 64) if 1 << p >= 2 * cap["strings"])
        model = Stream()
        lab, _ = check_call(s1, ss, model)
        lab.free()
        lab, want = check_call(s2, ss, model)
        decided(want)
        lab.free()
        info = ss.info()
        assert (info["strings"], info["bytes"]) == (info["capacity_strings"], info["capacity_bytes"]) == (cap["strings"], cap["bytes"])
    finally:
        ss.free(); s1.close(); s2.close()


def test_a_set_one_string_too_small_refuses_and_stays_as_it_was(pair):
    full = Stream()
    for f in pair["f"]:
        full.expect(f)
    cap = full.held_info()
    s1, s2 = sources(pair)
    small, fits = s1.sc.seen_set(cap["strings"] - 1, cap["bytes"]), s1.sc.seen_set(cap["strings"], cap["bytes"])
    short = s1.sc.seen_set(cap["strings"], cap["bytes"] - 8)
    try:
        for ss in (small, short, fits):
            model = Stream()
            lab, _ = check_call(s1, ss, model)
            lab.free()
            before = ss.info()
            if ss is fits:
                lab, _ = check_call(s2, ss, model)
                lab.free()
                continue
            out, info = C.c_void_p(0xDEAD0), sx.SeenInfo()
            assert sx.lib().sx_result_seen_device(s2.sc.h, s2.res.h, ss.h, 0, C.byref(out), C.byref(info)) == sx.SX_E_NOMEM and out.value is None
            text = sx.lib().sx_last_error(s2.sc.h).decode()
            assert "%d + %d strings of %d" % (before["strings"], cap["strings"] - before["strings"], before["capacity_strings"]) in text, text
            assert "%d + %d bytes of %d" % (before["bytes"], cap["bytes"] - before["bytes"], before["capacity_bytes"]) in text, text
            assert ss.info() == before
            lab, want = check_call(s2, ss, model, add=False)      # the set is as it was: the same words as a lookup in the model, and never refused
            decided(want)
            lab.free()
            assert ss.info() == before
    finally:
        small.free(); short.free(); fits.free(); s1.close(); s2.close()


def test_one_mission_results_of_unpacked_records():
    """the lane-per-region replay's segment: sx_finding records, strings where the writer put them; synth plants words of a short list
    in both buffers, and cuts some of them short"""
    ms = rc.missions(encodings=["utf-8"], chars_min="10")
    s1 = Source(ms, synth(random.Random(78), 2_000_000, 1 / 400), device_replay=True)
    s2 = Source(ms, synth(random.Random(79), 2_000_000, 1 / 400), device_replay=True)
    ss = s1.sc.seen_set(50_000, 8 << 20)
    try:
        assert not any(seg[4] for seg in s1.src + s2.src)
        model = Stream()
        lab, _ = check_call(s1, ss, model)
        lab.free()
        lab, want = check_call(s2, ss, model)
        decided(want)
        sel = s2.res.select_device(lab, any=FIRST, none=SEEN)
        check_selection(s2.sc, s2.src, sel, [f for f, w in zip(s2.all_f, want) if w & FIRST and not w & SEEN], s2.all_f, s2.ms, prints=False)
        sel.free(); lab.free()
    finally:
        ss.free(); s1.close(); s2.close()


def test_a_selections_output_as_the_source(pair):
    s1, s2 = sources(pair)
    ss = s1.sc.seen_set(100_000, 8 << 20)
    try:
        model = Stream()
        kept1, kept2 = filtered(s1.all_f, b"ab"), filtered(s2.all_f, b"ab")
        assert 0 < len(kept1) < len(s1.all_f) and 0 < len(kept2) < len(s2.all_f)
        sel1 = s1.res.select_device(b"ab")
        lab, _ = check_call(s1, ss, model, res=sel1, all_f=kept1)
        lab.free(); sel1.free()
        sel2 = s2.res.select_device(b"ab")
        lab, want = check_call(s2, ss, model, res=sel2, all_f=kept2)
        decided(want)
        new = sel2.select_device(lab, any=FIRST, none=SEEN)
        assert downloaded(s2.sc, new) == [f for f, w in zip(kept2, want) if w & FIRST and not w & SEEN]
        new.free(); lab.free(); sel2.free()
    finally:
        ss.free(); s1.close(); s2.close()


def raw_call(sc_h, res_h, set_h, flags=0, with_out=True):
    """the C entry point itself: (its code, *out afterwards — set to a sentinel before)"""
    out, info = C.c_void_p(0xDEAD0), sx.SeenInfo()
    rc_ = sx.lib().sx_result_seen_device(sc_h, res_h, set_h, flags, C.byref(out) if with_out else None, C.byref(info))
    return rc_, out.value


def test_refusals_leave_no_labels_and_the_set_as_it_was(pair):
    s1, s2 = sources(pair)
    sc, res = s1.sc, s1.res
    plain = sx.Scanner(pair["ms"], device=0)
    host = plain.scan(pair["data"][1], file_id=1)
    ss = sc.seen_set(100_000, 8 << 20)
    try:
        model = Stream()
        lab, _ = check_call(s2, ss, model)
        lab.free()
        before = ss.info()
        # bad flags, NULL arguments, a set of bad capacity
        for flags in (sx.SX_SELECT_ASCII_NOCASE, 2, sx.SX_SEEN_LOOKUP_ONLY | 1, 1 << 31):
            assert raw_call(sc.h, res.h, ss.h, flags) == (sx.SX_E_INVALID, None)
        assert raw_call(None, res.h, ss.h) == (sx.SX_E_INVALID, None) and raw_call(sc.h, None, ss.h) == (sx.SX_E_INVALID, None)
        assert raw_call(sc.h, res.h, None) == (sx.SX_E_INVALID, None) and raw_call(sc.h, res.h, ss.h, with_out=False)[0] == sx.SX_E_INVALID
        for cs, cb, flags in ((0, 1024, 0), ((1 << 40) + 1, 1024, 0), (16, (1 << 40) + 8, 0), (16, 1024, sx.SX_SELECT_INVERT)):
            out = C.c_void_p(0xDEAD0)
            assert sx.lib().sx_seen_set_create(sc.h, cs, cb, flags, C.byref(out)) == sx.SX_E_INVALID and out.value is None
        # a result in host memory; a freed set
        assert raw_call(plain.h, host.h, ss.h) == (sx.SX_E_STATE, None)
        assert "host memory" in sx.lib().sx_last_error(plain.h).decode()
        assert code_of(lambda: host.seen_device(ss)) == sx.SX_E_STATE
        gone = sc.seen_set(16, 1024)
        gone.free()
        assert code_of(lambda: res.seen_device(gone)) == sx.SX_E_INVALID and code_of(gone.info) == sx.SX_E_INVALID
        # a source whose block a later scan has reused
        res2 = sc.scan(pair["data"][0], file_id=1)
        assert raw_call(sc.h, res.h, ss.h) == (sx.SX_E_STATE, None)
        assert "reused" in sx.lib().sx_last_error(sc.h).decode()
        assert code_of(lambda: res.seen_device(ss)) == sx.SX_E_STATE
        res2.free()
        assert ss.info() == before
        # a host-only context has no device for it, neither for the call nor for a set
        host_only = sx.Scanner(pair["ms"], device=sx.SX_HOST_ONLY)
        assert raw_call(host_only.h, s2.res.h, ss.h) == (sx.SX_E_STATE, None)
        assert "host-only" in sx.lib().sx_last_error(host_only.h).decode()
        assert code_of(lambda: host_only.seen_set(16, 1024)) == sx.SX_E_STATE
        host_only.close()
        assert ss.info() == before
    finally:
        host.free(); plain.close(); res.free(); sc.close()
    # a closed Scanner; the set and the other context go on
    assert code_of(lambda: res.seen_device(ss)) == sx.SX_E_STATE
    try:
        lab, want = check_call(s2, ss, model)
        assert all(w & SEEN for w in want)
        lab.free()
    finally:
        ss.free(); s2.close()
