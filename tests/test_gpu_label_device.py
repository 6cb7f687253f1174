"""sx_label_set_create / sx_result_label_device / sx_result_select_labels_device (include/stringsext_amd.h): for every finding of a
result that lies in HBM WHICH patterns of a regex list its string holds, one 64-bit label per finding, made on the device
(stringsext_amd/csrc/sx_label_dev.hip), the findings per pattern counted on the way, and the selection by label.  The expected value
never comes from the code under test: a second Scanner without the flag scans the same data and Python's re.search says, per
pattern, which of its findings' strings hold it — every pattern rendered for Python with `$` as `\\Z`, folded sets with
re.IGNORECASE."""
import ctypes as C
import random
import re

import pytest

import refconfig as rc
import stringsext_amd as sx
from test_gpu_result_on_device_multi import case
from test_gpu_select_device import check_selection, downloaded, pointers
from test_gpu_select_regex_device import re_filtered
from test_gpu_select_set_device import Source, code_of
from test_host_logic import synth
from test_selre_core import to_python

pytestmark = pytest.mark.gpu

NEVER = sx.SX_LABEL_NEVER


def strings(findings):
    return [f["s"].encode("utf-8") for f in findings]


def py_labels(findings, pats, nocase=False):
    res = [re.compile(to_python(p), re.IGNORECASE if nocase else 0) for p in pats]
    return [sum(1 << p for p, r in enumerate(res) if r.search(s)) for s in strings(findings)]


def py_counters(labels, n_patterns, base=0):
    findings = [sum(lab >> p & 1 for lab in labels) for p in range(n_patterns)]
    first = [next((base + i for i, lab in enumerate(labels) if lab >> p & 1), NEVER) for p in range(n_patterns)]
    return findings, first


def decided(labels, n_patterns):
    """every pattern hits at least one finding and fewer than all: the inputs cannot hide an empty comparison"""
    counts = py_counters(labels, n_patterns)[0]
    assert all(0 < c < len(labels) for c in counts), counts
    return counts


def middle(findings):
    """two bytes from the middle of one of the case's strings"""
    d = sorted({s for s in strings(findings) if len(s) >= 6})
    mid = d[len(d) // 3]
    return mid[(len(mid) - 2) // 2:(len(mid) - 2) // 2 + 2]


def data_patterns(findings):
    """six patterns from the case's own strings: a head, a tail, a middle, a length, a span, and a head with a tail"""
    d = sorted({s for s in strings(findings) if len(s) >= 6})
    q1, q2, mid = d[len(d) // 4], d[len(d) // 2], d[len(d) // 3]
    return [b"^" + re.escape(q1[:1]), re.escape(q2[-1:]) + b"$", re.escape(middle(findings)), b"^.{0,20}$",
            re.escape(q1[:1]) + b".+" + re.escape(q2[-1:]), b"^(?:" + re.escape(q1[:1]) + b"|" + re.escape(mid[:1]) + b").*[a-m]$"]


def picked(label, any_, all_, none):
    return (any_ == 0 or label & any_ != 0) and label & all_ == all_ and label & none == 0


def flat(lab, src):
    """a Labels object's words in print order; an array per source segment, of the segment's size"""
    segs = lab.device_segments()
    assert [n for _, n in segs] == [s[1] for s in src] and all(p and p % 256 == 0 for p, _ in segs)
    return [w for seg in lab.download() for w in seg]


@pytest.fixture(scope="module")
def case_d():
    """case "D" — one Mission with findings among two — with its findings of two buffers of one stream"""
    ms, data, _ = case("D")
    ref = sx.Scanner(ms, device=0)
    host = ref.scan(data, file_id=1)
    all_f = host.findings()
    host2 = ref.scan(data, file_id=1)
    all_f2 = host2.findings()
    host.free(); host2.free(); ref.close()
    assert len(all_f) > 1000 and len(all_f2) > 1000
    return dict(ms=ms, data=data, all_f=all_f, all_f2=all_f2)


def labels_counters_and_the_selection_by_label(name, ms, data, device_replay=None, packed=True):
    s = Source(ms, data, device_replay=device_replay)
    try:
        assert all(seg[4] == packed for seg in s.src)
        pats = data_patterns(s.all_f)
        want = py_labels(s.all_f, pats)
        counts = decided(want, len(pats))
        print(name, len(want), pats, counts)
        ls = s.sc.label_set(pats)
        info = ls.info
        assert (info.n_patterns, info.nocase) == (len(pats), 0) and info.lds_states == info.states and 0 < info.here_states < info.states
        assert ls.read() == ([0] * len(pats), [NEVER] * len(pats))                   # a new set is reset
        lab = s.res.label_device(ls, ordinal_base=5)
        got = flat(lab, s.src)
        assert got == want, next((i, hex(a), hex(b), s.all_f[i]["s"]) for i, (a, b) in enumerate(zip(got, want)) if a != b)
        assert ls.read() == py_counters(want, len(pats), base=5)
        assert pointers(s.res) == s.before                                           # read, not moved
        # the selection by label: `any`, `all`, `none`, and all three at once
        for any_, all_, none in ((0b000101, 0, 0), (0, 0b001001, 0), (0, 0, 0b010110), (0b000011, 0b001000, 0b100000)):
            kept = [f for f, w in zip(s.all_f, want) if picked(w, any_, all_, none)]
            assert 0 < len(kept) < len(want), (any_, all_, none, len(kept))
            sel = s.res.select_device(lab, any=any_, all=all_, none=none)
            check_selection(s.sc, s.src, sel, kept, s.all_f, s.ms, prints=False)     # (downloaded() checks the layout rule with download_segment)
            sel.free()
        # mask bits the set does not have: in `all` nothing, in `none` harmless; the empty result
        nothing = s.res.select_device(lab, all=1 << 63)
        assert len(nothing) == 0 and nothing.device_segments() == [] and nothing.findings() == []
        everything = s.res.select_device(lab, none=1 << 40)
        assert len(everything) == len(want)
        everything.free()
        everything = s.res.select_device(lab)
        assert len(everything) == len(want) and [seg[1] for seg in everything.device_segments()] == [seg[1] for seg in s.src]
        nothing.free(); everything.free(); lab.free(); ls.free()
    finally:
        s.close()


@pytest.mark.parametrize("name", ["A", "C", "D"])
def test_several_missions(name):
    """the merger's segments: sx_finding16 records, the strings of a segment in one range"""
    ms, data, _ = case(name)
    labels_counters_and_the_selection_by_label(name, ms, data)


def test_one_mission_sparse_unpacked_segment():
    """the lane-per-region replay's segment: sx_finding records, strings where the writer put them"""
    data = synth(random.Random(78), 4_000_000, 1 / 400)
    labels_counters_and_the_selection_by_label("sparse", rc.missions(encodings=["utf-8"], chars_min="10"), data, device_replay=True, packed=False)


def test_the_fold(case_d):
    d = case_d
    s = Source(d["ms"], d["data"], all_f=d["all_f"])
    try:
        pats = [p for p in data_patterns(d["all_f"]) if re.search(rb"[A-Za-z]", p)] + [b"^[a-f]+[0-9]", b"[G-H]{2}$"]
        want, plain = py_labels(d["all_f"], pats, nocase=True), py_labels(d["all_f"], pats)
        decided(want, len(pats))
        assert sum(bin(w).count("1") for w in want) > sum(bin(w).count("1") for w in plain)      # the fold decides something
        ls = s.sc.label_set(pats, ignore_case=True)
        assert ls.info.nocase == 1
        lab = s.res.label_device(ls)
        assert flat(lab, s.src) == want and ls.read() == py_counters(want, len(pats))
        lab.free(); ls.free()
    finally:
        s.close()


def test_a_set_of_64_patterns_and_a_set_of_one(case_d):
    d = case_d
    s = Source(d["ms"], d["data"], all_f=d["all_f"])
    try:
        uniq = sorted({x for x in strings(d["all_f"]) if len(x) >= 6})
        pats = [re.escape(uniq[k * len(uniq) // 62][2:4]) for k in range(62)] + [b"^" + re.escape(uniq[7][:2]), re.escape(uniq[-9][-2:]) + b"$"]
        want = py_labels(d["all_f"], pats)
        decided(want, 64)
        assert any(w >> 63 for w in want) and any(w >> 32 and not w & 0xFFFFFFFF for w in want)
        ls = s.sc.label_set(pats)
        print(ls.info.states, ls.info.classes, ls.info.lds_states, ls.info.here_states)
        lab = s.res.label_device(ls)
        assert flat(lab, s.src) == want and ls.read() == py_counters(want, 64)
        kept = [f for f, w in zip(d["all_f"], want) if w >> 63]
        sel = s.res.select_device(lab, any=1 << 63)
        assert downloaded(s.sc, sel) == kept
        sel.free(); lab.free(); ls.free()
        # one pattern: the label is the regex selection's bit
        one = [pats[62]]
        ls = s.sc.label_set(one)
        lab = s.res.label_device(ls)
        got = flat(lab, s.src)
        members = {id(f) for f in re_filtered(d["all_f"], one)}
        assert got == [int(id(f) in members) for f in d["all_f"]] and 0 < len(members) < len(got)
        lab.free(); ls.free()
    finally:
        s.close()


def test_two_buffers_add_up_and_reset_forgets(case_d):
    d = case_d
    s = Source(d["ms"], d["data"], all_f=d["all_f"])
    try:
        n, pats = len(d["all_f"]), data_patterns(d["all_f"])
        one, two = py_labels(d["all_f"], pats), py_labels(d["all_f2"], pats)
        ls = s.sc.label_set(pats)
        lab1 = s.res.label_device(ls)
        res2 = s.sc.scan(d["data"], file_id=1)                                      # the stream's second buffer on the same Scanner
        assert len(res2) == len(two)
        lab2 = res2.label_device(ls, ordinal_base=n)
        assert flat(lab2, res2.device_segments()) == two
        assert ls.read() == py_counters(one + two, len(pats))
        d_findings, d_first = ls.counters_device()
        raw = s.sc.download(C.c_void_p(d_findings), 64 * 8) + s.sc.download(C.c_void_p(d_first), 64 * 8)
        words = list((C.c_uint64 * 128).from_buffer_copy(raw))
        assert (words[:len(pats)], words[64:64 + len(pats)]) == ls.read() and words[len(pats):64] == [0] * (64 - len(pats))
        assert lab1.download() and lab1.device_segments()                           # the first buffer's labels are their own memory: still there
        ls.reset()
        assert ls.read() == ([0] * len(pats), [NEVER] * len(pats))
        lab3 = res2.label_device(ls, ordinal_base=n)
        assert ls.read() == py_counters(two, len(pats), base=n)
        for x in (lab1, lab2, lab3, res2, ls):
            x.free()
    finally:
        s.res.free(); s.sc.close()


def test_a_selection_and_an_extraction_are_sources_and_labelling_ages_no_selection():
    ms, data, _ = case("C")
    s = Source(ms, data)
    try:
        all_f, res, sc = s.all_f, s.res, s.sc
        pats = data_patterns(all_f)
        ls = sc.label_set(pats)
        # a regex selection as the source
        shape = [b"^.{0,20}$", pats[2]]
        kept = re_filtered(all_f, shape)
        assert 0 < len(kept) < len(all_f)
        rs = sc.regex_set(shape)
        sel = res.select_device(rs)
        want = py_labels(kept, pats)
        assert any(want) and len(set(want)) > 2
        lab = sel.label_device(ls, ordinal_base=3)
        assert flat(lab, sel.device_segments()) == want and ls.read() == py_counters(want, len(pats), base=3)
        # ... and selecting from the selection by its labels
        sub = sel.select_device(lab, any=1 << 2)
        assert downloaded(sc, sub) == [f for f, w in zip(kept, want) if w >> 2 & 1]
        lab.free(); sub.free()
        # an extraction as the source: its matches are findings
        cut = [rb"[0-9]{2,}", rb"[A-F]+="]      # (runs of one class, the second closed by a byte outside it: leftmost-longest is what re.finditer finds)
        matches = [dict(f, s=m.group().decode("utf-8")) for f in all_f for m in re.finditer(rb"[0-9]{2,}|[A-F]+=", f["s"].encode("utf-8"))]
        xs = sc.extract_set(cut)
        ext = res.extract_device(xs)
        assert len(ext) == len(matches) > 100
        kinds = [b"^[0-9]", b"=$", b"[0-9]{3}"]
        want = py_labels(matches, kinds)
        decided(want, 3)
        ks = sc.label_set(kinds)
        lab = ext.label_device(ks)
        assert flat(lab, ext.device_segments()) == want and ks.read() == py_counters(want, 3)
        lab.free(); ks.free(); xs.free(); rs.free()
        # labelling is no selection: `sel` was made two selections ago (sub, ext) and would be stale after a third one; labellings do not count
        mid = middle(all_f)
        s1 = res.select_device(mid)
        for _ in range(3):
            res.label_device(ls).free()
        s2 = res.select_device(mid[:1])
        for _ in range(3):
            s1.label_device(ls).free()
        assert downloaded(sc, s1) == [f for f in all_f if mid in f["s"].encode("utf-8")]      # a selection, labellings, a selection, labellings: still there
        s3 = res.select_device(mid[1:])
        assert code_of(lambda: s1.label_device(ls)) == sx.SX_E_STATE                # the second selection behind it has taken its block
        for x in (sel, ext, s1, s2, s3, ls):
            x.free()
    finally:
        s.close()


def test_labels_of_another_result_a_reused_source_and_a_host_only_context(case_d):
    d = case_d
    s = Source(d["ms"], d["data"], all_f=d["all_f"])
    sc, res = s.sc, s.res
    try:
        pats = data_patterns(d["all_f"])
        ls = sc.label_set(pats)
        lab = res.label_device(ls)
        want = py_counters(py_labels(d["all_f"], pats), len(pats))
        sel = res.select_device(lab, any=1)
        # labels made from another result
        assert code_of(lambda: sel.select_device(lab, any=1)) == sx.SX_E_INVALID
        assert "not made from this result" in sx.lib().sx_last_error(sc.h).decode()
        lab_sel = sel.label_device(ls)
        assert code_of(lambda: res.select_device(lab_sel, any=1)) == sx.SX_E_INVALID
        ls.reset()
        # the masks belong to Labels, the flags do not
        with pytest.raises(ValueError):
            res.select_device(lab, invert=True)
        with pytest.raises(ValueError):
            res.select_device(b"ab", any=1)
        with pytest.raises(TypeError):
            res.extract_device(ls)
        # an empty selection is in host memory, as every result without findings; a host result of a Scanner without the flag
        none = res.select_device(lab, all=1 << 63)
        assert len(none) == 0 and code_of(lambda: none.label_device(ls)) == sx.SX_E_STATE
        plain = sx.Scanner(d["ms"], device=0)
        host = plain.scan(d["data"], file_id=1)
        assert code_of(lambda: host.label_device(ls)) == sx.SX_E_STATE
        assert code_of(lambda: host.select_device(lab, any=1)) == sx.SX_E_STATE     # in host memory, and not the labels' result: the first refusal wins
        host.free(); plain.close(); none.free()
        # a source whose block a later scan has reused: to label it and to select by its labels
        res2 = sc.scan(d["data"], file_id=1)
        assert code_of(lambda: res.label_device(ls)) == sx.SX_E_STATE
        assert code_of(lambda: res.select_device(lab, any=1)) == sx.SX_E_STATE
        assert ls.read() == ([0] * len(pats), [NEVER] * len(pats))                  # nothing of all that was counted
        assert code_of(lambda: res2.select_device(lab, any=1)) == sx.SX_E_INVALID   # the same place in HBM, another result
        # a freed set, freed labels
        gone = sc.label_set(pats)
        gone.free(); gone.free()
        assert code_of(lambda: res2.label_device(gone)) == sx.SX_E_INVALID and code_of(gone.read) == sx.SX_E_INVALID
        lab_sel.free(); lab_sel.free()
        assert code_of(lambda: sel.select_device(lab_sel)) == sx.SX_E_INVALID
        sel.free(); res2.free()
    finally:
        res.free(); sc.close()
    # a host-only context compiles the patterns and has no device for them
    host_only = sx.Scanner(d["ms"], device=sx.SX_HOST_ONLY)
    assert code_of(lambda: host_only.label_set(pats)) == sx.SX_E_STATE
    assert code_of(lambda: host_only.label_set([b"a**"])) == sx.SX_E_INVALID
    host_only.close()
    # a closed Scanner; the set and the labels are still there, and another Scanner on the same device counts into the set
    assert code_of(lambda: res.label_device(ls)) == sx.SX_E_STATE
    assert ls.info.n_patterns == len(pats) and len(lab.device_segments()) >= 1
    other = sx.Scanner(d["ms"], device=0, result_on_device=True)
    theirs = other.scan(d["data"], file_id=1)
    lab2 = theirs.label_device(ls)
    assert ls.read() == want
    for x in (lab, lab2, theirs):
        x.free()
    other.close()
    assert ls.read() == want
    ls.free()
