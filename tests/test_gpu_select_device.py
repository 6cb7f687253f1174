"""sx_result_select_device (include/stringsext_amd.h): the findings of a result that lies in HBM, selected by substring on the device
(stringsext_amd/csrc/sx_select_dev.hip).  The expected value never comes from the code under test: a second Scanner without the
flag scans the same data — its findings() equal the oracle's text, as tests/test_gpu_result_on_device_multi.py asserts — and
Python filters them with the header's match rule.  The patterns are taken from the data."""
import ctypes as C
import random

import pytest

import refconfig as rc
import stringsext_amd as sx
import sxo_binding as sxo
from test_gpu_result_on_device_multi import case, download_segment, expanded
from test_host_logic import synth
from test_print_core import print_finding
from test_wave_core import text_lines

pytestmark = pytest.mark.gpu

CANNOT_OCCUR = b"zzzzzzzz"
PRECISION_CODE = {v: k for k, v in sx.PRECISION.items()}
FORMATS = ((None, False), ("x", False), ("d", False), ("o", False), ("x", True))


def matches(s, patterns, ignore_case):
    """the header's rule with Python's substring search (bytes.lower() folds 'A'..'Z' and nothing else)"""
    if ignore_case:
        s, patterns = s.lower(), [p.lower() for p in patterns]
    return any(p in s for p in patterns)


def filtered(findings, patterns, ignore_case=False, invert=False):
    patterns = [patterns] if isinstance(patterns, bytes) else patterns
    return [f for f in findings if matches(f["s"].encode("utf-8"), patterns, ignore_case) != invert]


def middle3(s):
    return s[(len(s) - 3) // 2:(len(s) - 3) // 2 + 3]


def pick_patterns(findings):
    """the pattern sets of a case, from its own strings: {name: (patterns, ignore_case)}"""
    strs = [f["s"].encode("utf-8") for f in findings]
    med = strs[len(strs) // 2]
    two = b"7g" if any(b"7g" in s for s in strs) else med[1:3]
    in_how_many = {b: sum(1 for s in strs if bytes([b]) in s) for b in set(med)}
    one = bytes([min(in_how_many, key=lambda b: (in_how_many[b], b))])       # the median string's rarest byte
    return {"three": (middle3(med), False), "eight": (med[:8], False), "two": (two, False), "two nocase": (two, True), "one": (one, False),
            "sixteen": ([middle3(strs[k * len(strs) // 16]) for k in range(16)], False)}


def labels(ms):
    return [(m["mission_id"], b"ascii" if m["print_encoding_as_ascii"] else sx.encoding_name(m["encoding"]).encode()) for m in ms]


def printed_by_python(findings, ms, radix, no_metadata):
    lab = labels(ms)
    return b"".join(print_finding(dict(f, precision=PRECISION_CODE[f["precision"]], s=f["s"].encode("utf-8")), 1, radix, no_metadata, lab)
                    for f in findings)


def pointers(res):
    return [(s[0], s[1], s[2], s[3], s[4]) for s in res.device_segments()]


def info_tuple(info):
    return (info.packed, info.input_file_id, info.slice_base, tuple(info.position0))


def downloaded(sc, sel):
    got = []
    for seg in sel.device_segments():
        assert seg[0] is not None and seg[0] % 256 == 0 and seg[2] == seg[0] + seg[1] * (16 if seg[4] else 32)   # [records][strings], 256-byte aligned
        recs, arena = download_segment(sc, seg)          # (checks the layout rule: the strings back to back in record order)
        got += expanded(recs, arena, seg[4], seg[5])
    return got


def check_selection(sc, src_segs, sel, want, all_findings, ms, prints=True):
    """sel against the filtered list `want` of all_findings, the source's findings, whose segments are src_segs"""
    assert len(sel) == len(want)
    segs = sel.device_segments()
    # every source segment with a selected finding gives one segment: its records in order, its record type, its sx_segment_info
    ids = {id(f) for f in want}
    at, expect = 0, []
    for s in src_segs:
        k = sum(1 for f in all_findings[at:at + s[1]] if id(f) in ids)
        at += s[1]
        if k:
            expect.append((k, s[4], info_tuple(s[5])))
    assert at == len(all_findings)
    assert [(s[1], s[4], info_tuple(s[5])) for s in segs] == expect
    got = downloaded(sc, sel)
    assert got == want, next(((a, b) for a, b in zip(got, want) if a != b), (len(got), len(want)))
    if not prints:
        return
    text_x = None
    for radix, no_metadata in FORMATS:
        p, n = sel.printed_device(n_inputs=1, radix=radix, no_metadata=no_metadata)
        text = sc.download(C.c_void_p(p), n)
        assert text == printed_by_python(want, ms, radix, no_metadata), (radix, no_metadata)
        text_x = text if (radix, no_metadata) == ("x", False) else text_x
    assert pointers(sel) == [(s[0], s[1], s[2], s[3], s[4]) for s in segs]           # printing moves nothing
    assert sel.printed(n_inputs=1, radix="x") == text_x                               # the host accessors fetch it, as a scan's
    assert sel.findings() == want


def run_case(ms, data, device_replay=None, min_segments=1, packed=None, min_findings=100):
    want_text = sxo.run_cli(ms, [data], radix="x")
    ref = sx.Scanner(ms, device=0, device_replay=device_replay)
    sc = sx.Scanner(ms, device=0, device_replay=device_replay, result_on_device=True)
    try:
        host = ref.scan(data, file_id=1)
        all_f = host.findings()
        assert len(all_f) >= min_findings
        res = sc.scan(data, file_id=1)
        src = res.device_segments()
        before = pointers(res)
        assert len(src) >= min_segments and all(s[0] is not None for s in src) and sum(s[1] for s in src) == len(all_f)
        if packed is not None:
            assert all(s[4] == packed for s in src)
        sets = pick_patterns(all_f)
        for name, (pats, nocase) in sets.items():
            want = filtered(all_f, pats, nocase)
            print(f"{name}: {pats!r} selects {len(want)} of {len(all_f)}")
            assert 0 < len(want) < len(all_f), (name, pats, len(want))
            sel = res.select_device(pats, ignore_case=nocase)
            check_selection(sc, src, sel, want, all_f, ms)
            sel.free()
        assert len(filtered(all_f, *sets["two nocase"])) >= len(filtered(all_f, *sets["two"]))
        # INVERT and the plain selection partition the source
        pats = sets["three"][0]
        plain, inverse = res.select_device(pats), res.select_device(pats, invert=True)
        assert len(plain) + len(inverse) == len(res)
        check_selection(sc, src, inverse, filtered(all_f, pats, invert=True), all_f, ms)
        check_selection(sc, src, plain, filtered(all_f, pats), all_f, ms, prints=False)
        plain.free(); inverse.free()
        # selecting from a selection is AND
        a, b = sets["one"][0], sets["three"][0]       # (the median finding holds both)
        first = res.select_device(a)
        first_segs, first_ptrs = first.device_segments(), pointers(first)
        second = first.select_device(b, ignore_case=True)
        both = filtered(filtered(all_f, a), b, ignore_case=True)
        assert both == [f for f in all_f if a in f["s"].encode() and b.lower() in f["s"].encode().lower()]
        assert 0 < len(both) < len(first)
        check_selection(sc, first_segs, second, both, filtered(all_f, a), ms)
        assert pointers(first) == first_ptrs
        first.free(); second.free()
        # nothing selected: an empty result, which is in host memory as every result without findings
        assert filtered(all_f, CANNOT_OCCUR) == []
        none = res.select_device(CANNOT_OCCUR)
        assert len(none) == 0 and none.device_segments() == [] and none.segments() == [] and none.findings() == []
        with pytest.raises(sx.SxError) as e:
            none.printed_device(radix="x")
        assert e.value.code == sx.SX_E_STATE
        with pytest.raises(sx.SxError) as e:
            none.select_device(b"a")
        assert e.value.code == sx.SX_E_STATE
        everything = res.select_device(CANNOT_OCCUR, invert=True)
        check_selection(sc, src, everything, all_f, all_f, ms, prints=False)
        none.free(); everything.free()
        # the source was read, not moved, and still prints the oracle's full text
        assert pointers(res) == before
        p, n = res.printed_device(n_inputs=1, radix="x")
        assert sx.OUTPUT_BOM + sc.download(C.c_void_p(p), n) + b"\n" == want_text
        assert pointers(res) == before
        assert sx.OUTPUT_BOM + res.printed(n_inputs=1, radix="x") + b"\n" == want_text
        res.free(); host.free()
        return len(src)
    finally:
        sc.close(); ref.close()


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_several_missions(name):
    ms, data, _ = case(name)
    run_case(ms, data, min_findings=100)


def test_one_mission_dense_packed_segment(monkeypatch):
    """the wave path's segment: sx_finding16 records, strings where the writer put them — the selection's are back to back"""
    monkeypatch.setenv("SX_WAVE_REPLAY", "1")
    data = text_lines(random.Random(77), 3_000_000)
    assert run_case(rc.missions(encodings=["ascii"], chars_min="4"), data, packed=True) == 1


def test_one_mission_sparse_unpacked_segment():
    """the lane-per-region replay's segment: sx_finding records"""
    data = synth(random.Random(78), 8_000_000, 1 / 400)
    run_case(rc.missions(encodings=["utf-8"], chars_min="10"), data, device_replay=True, packed=False)


def test_unpacked_merger_records(monkeypatch):
    monkeypatch.setenv("SX_PACKED", "0")
    ms, data, _ = case("A")
    run_case(ms, data, packed=False)


def test_several_parts_are_several_segments(monkeypatch):
    monkeypatch.setenv("SX_MERGE_PART_FINDINGS", "7000")
    monkeypatch.setenv("SX_MERGE_PART_MIB", "1")
    ms, data, _ = case("A")
    assert run_case(ms, data, min_segments=3) >= 3


def code_of(call):
    with pytest.raises(sx.SxError) as e:
        call()
    return e.value.code


def test_a_selection_lives_until_the_second_selection_after_it_and_through_scans():
    ms, data, _ = case("A")
    ref = sx.Scanner(ms, device=0)
    sc = sx.Scanner(ms, device=0, result_on_device=True)
    try:
        host = ref.scan(data, file_id=1)
        all_f = host.findings()
        sets = pick_patterns(all_f)
        pa, pb, pc = sets["three"][0], sets["two"][0], sets["eight"][0]
        res = sc.scan(data, file_id=1)
        src = res.device_segments()
        s1 = res.select_device(pa)
        s2 = res.select_device(pb)
        check_selection(sc, src, s1, filtered(all_f, pa), all_f, ms, prints=False)       # one selection later: still there
        assert {s[0] for s in s1.device_segments()}.isdisjoint({s[0] for s in s2.device_segments()})
        s3 = res.select_device(pc)
        assert code_of(s1.device_segments) == sx.SX_E_STATE                                # the third selection has taken its block
        assert code_of(s1.segments) == sx.SX_E_STATE
        assert code_of(lambda: s1.printed_device(radix="x")) == sx.SX_E_STATE
        assert code_of(lambda: s1.select_device(pa)) == sx.SX_E_STATE
        # s2's block is the one the next selection writes: it cannot be that selection's source — and a refused call does not count
        assert code_of(lambda: s2.select_device(pa)) == sx.SX_E_STATE
        assert code_of(lambda: res.select_device(b"")) == sx.SX_E_INVALID
        check_selection(sc, src, s2, filtered(all_f, pb), all_f, ms, prints=False)
        # a scan in between does not invalidate a selection ...
        res2 = sc.scan(data[:4096 * 100], file_id=1)
        assert all(s[0] is not None for s in res2.device_segments())
        p, n = s3.printed_device(n_inputs=1, radix="x")
        assert sc.download(C.c_void_p(p), n) == printed_by_python(filtered(all_f, pc), ms, "x", False)
        s4 = s3.select_device(pc[:2])                                                      # (this one does take s2's block)
        check_selection(sc, s3.device_segments(), s4, filtered(filtered(all_f, pc), pc[:2]), filtered(all_f, pc), ms, prints=False)
        check_selection(sc, src, s3, filtered(all_f, pc), all_f, ms)
        assert code_of(s2.device_segments) == sx.SX_E_STATE
        # ... but it does invalidate the source
        assert code_of(lambda: res.select_device(pa)) == sx.SX_E_STATE
        assert code_of(res.device_segments) == sx.SX_E_STATE
        for r in (s1, s2, s3, s4, res, res2, host):
            r.free()
    finally:
        sc.close(); ref.close()


def test_a_moved_segment_a_result_in_host_memory_and_a_closed_scanner_are_refused():
    ms, data, _ = case("D")
    # a Scanner without the flag: the caller filters on the host
    sc = sx.Scanner(ms, device=0)
    res = sc.scan(data, file_id=1)
    assert len(res) > 100 and code_of(lambda: res.select_device(b"e")) == sx.SX_E_STATE
    out = C.c_void_p(1)
    arr = (sx.Pattern * 1)(sx.Pattern(b"e", 1))
    assert sx.lib().sx_result_select_device(sc.h, res.h, arr, 1, 0, C.byref(out)) == sx.SX_E_STATE and out.value is None
    res.free(); sc.close()
    sc = sx.Scanner(ms, device=0, result_on_device=True)
    # no findings at all
    res = sc.scan(bytes(1 << 20), file_id=1)
    assert len(res) == 0 and code_of(lambda: res.select_device(b"e")) == sx.SX_E_STATE
    res.free()
    # bad arguments are told apart from that
    res = sc.scan(data, file_id=1)
    for bad in ([], [b"x"] * 17, [b""], [b"y" * 65]):
        assert code_of(lambda: res.select_device(bad)) == sx.SX_E_INVALID
    assert sx.lib().sx_result_select_device(sc.h, res.h, arr, 1, 4, C.byref(out)) == sx.SX_E_INVALID and out.value is None
    sel = res.select_device([b"E"] * 16, ignore_case=True)                # 16 patterns and 64 bytes are the limits
    long_one = res.select_device(b"y" * 64)
    assert len(sel) > 0 and len(long_one) == 0
    # a segment a host accessor has moved
    fp, n, ap, alen = C.POINTER(sx.Finding)(), C.c_uint64(), C.POINTER(C.c_uint8)(), C.c_uint64()
    sc._chk(sx.lib().sx_result_segment(res.h, 0, C.byref(fp), C.byref(n), C.byref(ap), C.byref(alen)))
    assert res.device_segments()[0][0] is None
    assert code_of(lambda: res.select_device(b"e")) == sx.SX_E_STATE
    assert all(s[0] is not None for s in sel.device_segments())         # (the selection made before is its own memory)
    # a result of another Scanner: its memory is not this context's
    other = sx.Scanner(ms, device=0, result_on_device=True)
    theirs = other.scan(data, file_id=1)
    assert sx.lib().sx_result_select_device(sc.h, theirs.h, arr, 1, 0, C.byref(out)) == sx.SX_E_STATE and out.value is None
    theirs.free(); other.close()
    # a closed Scanner
    res2 = sc.scan(data, file_id=1)
    sel2 = res2.select_device(b"e")
    assert len(sel2) > 0
    sc.close()
    assert code_of(lambda: res2.select_device(b"e")) == sx.SX_E_STATE
    assert code_of(sel2.device_segments) == sx.SX_E_STATE
    assert code_of(sel.segments) == sx.SX_E_STATE
    for r in (res, res2, sel, sel2, long_one):
        r.free()
