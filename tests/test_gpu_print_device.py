"""sx_print_findings_device (include/stringsext_amd.h): Finding::print for a result that lies in HBM, written by the device
(stringsext_amd/csrc/sx_print_dev.hip).  Every case is compared, byte for byte, with the ORACLE's text (and, for two inputs, with
sx_print_findings of a Scanner without the flag); the result must stay where it is; every state in which the result is not on the
device must be refused with SX_E_STATE."""
import ctypes as C
import random
import re

import numpy as np
import pytest

import refconfig as rc
import stringsext_amd as sx
import sxo_binding as sxo
from test_gpu_result_on_device_multi import C5, F16, case
from test_host_logic import synth
from test_wave_core import text_lines

pytestmark = pytest.mark.gpu

C5_LABELS = {0: b"UTF-8", 1: b"UTF-16LE", 2: b"UTF-16BE", 3: b"Big5", 4: b"EUC-JP", 5: b"KOI8-R"}   # Encoding::name()


def device_text(sc, res, **kw):
    p, n = res.printed_device(**kw)
    assert p and n
    return sc.download(C.c_void_p(p), n)


def pointers(res):
    return [(s[0], s[1], s[2], s[3], s[4]) for s in res.device_segments()]


def check_print(ms, data, device_replay=None, min_segments=1, packed=None):
    ref = sx.Scanner(ms, device=0, device_replay=device_replay)
    sc = sx.Scanner(ms, device=0, device_replay=device_replay, result_on_device=True)
    try:
        res = sc.scan(data, file_id=1)
        before = pointers(res)
        assert len(before) >= min_segments and all(s[0] is not None for s in before), before
        if packed is not None:
            assert all(s[4] == packed for s in before)
        want_x = None
        for radix, no_metadata in ((None, False), ("x", False), ("d", False), ("o", False), ("x", True)):
            want = sxo.run_cli(ms, [data], radix=radix, no_metadata=no_metadata)                     # the oracle's text
            got = sx.OUTPUT_BOM + device_text(sc, res, n_inputs=1, radix=radix, no_metadata=no_metadata) + b"\n"
            assert len(got) == len(want) and got == want, (radix, no_metadata, len(got), len(want))
            want_x = want if (radix, no_metadata) == ("x", False) else want_x
        assert len(want_x) > 1000
        # two inputs: the file letter, which a one-file oracle run does not reach
        host = ref.scan(data, file_id=1)
        assert device_text(sc, res, n_inputs=2, radix="x") == host.printed(n_inputs=2, radix="x")
        assert b"\nA " in host.printed(n_inputs=2, radix="x")[:200]
        # the result was not moved, and the host accessors still work
        assert pointers(res) == before
        assert sx.OUTPUT_BOM + res.printed(n_inputs=1, radix="x") + b"\n" == want_x
        res.free(); host.free()
        # ... and no file id (stdin)
        sc.reset(); ref.reset()
        res, host = sc.scan(data, file_id=-1), ref.scan(data, file_id=-1)
        assert all(s[0] is not None for s in res.device_segments())
        assert device_text(sc, res, n_inputs=2, radix="x") == host.printed(n_inputs=2, radix="x") == want_x[3:-1]
        res.free(); host.free()
        return len(before)
    finally:
        sc.close(); ref.close()


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_several_missions(name):
    ms, data, _ = case(name)
    check_print(ms, data)


def test_one_mission_dense_packed_segment(monkeypatch):
    """the wave path's segment: sx_finding16 records, strings where the writer put them"""
    monkeypatch.setenv("SX_WAVE_REPLAY", "1")
    rng = random.Random(77)
    data = text_lines(rng, 3_000_000)
    for kw in (dict(encodings=["ascii"], chars_min="4"), dict(encodings=["utf-8"], chars_min="10", grep_char="58"),
               dict(encodings=["utf-16le"], chars_min="4")):
        d = data.decode("latin-1").encode("utf-16-le") if kw["encodings"][0].startswith("utf-16") else data
        assert check_print(rc.missions(**kw), d, packed=True) == 1


def test_one_mission_sparse_unpacked_segment():
    """the lane-per-region replay's segment: sx_finding records, the file id in every record"""
    rng = random.Random(78)
    data = synth(rng, 8_000_000, 1 / 400)
    check_print(rc.missions(encodings=["utf-8"], chars_min="10"), data, device_replay=True, packed=False)


def test_unpacked_merger_records(monkeypatch):
    monkeypatch.setenv("SX_PACKED", "0")
    ms, data, _ = case("A")
    check_print(ms, data, packed=False)


def test_the_text_runs_across_several_segments_without_a_seam(monkeypatch):
    monkeypatch.setenv("SX_MERGE_PART_FINDINGS", "7000")
    monkeypatch.setenv("SX_MERGE_PART_MIB", "1")
    ms, data, _ = case("A")
    assert check_print(ms, data, min_segments=3) >= 3


def test_positions_with_all_their_digits():
    """counter_offset 0xF000000000000000 in every Mission (the same origin: the result stays on the device)"""
    ms, data, _ = case("A")
    ms = [dict(m, counter_offset=0xF000000000000000) for m in ms]
    check_print(ms, data)
    sc = sx.Scanner(ms, device=0, result_on_device=True)
    try:
        res = sc.scan(data, file_id=1)
        assert re.match(rb"\n[ <>]f[0-9a-f]{15}[ +]\t\([a-d] ", device_text(sc, res, radix="x"))
        assert re.match(rb"\n[ <>]1[0-9]{19}[ +]\t\([a-d] ", device_text(sc, res, radix="d"))
        assert re.match(rb"\n[ <>]1[0-7]{21}[ +]\t\([a-d] ", device_text(sc, res, radix="o"))
        res.free()
    finally:
        sc.close()


def refused(res, **kw):
    with pytest.raises(sx.SxError) as e:
        res.printed_device(**kw)
    return e.value.code


def test_an_unknown_radix_is_invalid():
    ms, data, _ = case("D")
    sc = sx.Scanner(ms, device=0, result_on_device=True)
    try:
        res = sc.scan(data, file_id=1)
        assert refused(res, radix="q") == sx.SX_E_INVALID
        p, n = C.c_void_p(1), C.c_uint64(1)
        assert sx.lib().sx_print_findings_device(sc.h, res.h, 1, ord("X"), 0, C.byref(p), C.byref(n)) == sx.SX_E_INVALID
        assert p.value is None and n.value == 0
        assert device_text(sc, res, radix="x") == res.printed(radix="x")     # (the result is still good)
        res.free()
    finally:
        sc.close()


def test_a_result_in_host_memory_is_refused(monkeypatch):
    ms, data, _ = case("A")
    want = sxo.run_cli(ms, [data], radix="x")
    # a Scanner without the flag
    sc = sx.Scanner(ms, device=0)
    res = sc.scan(data, file_id=1)
    assert refused(res, radix="x") == sx.SX_E_STATE
    p, n = C.c_void_p(1), C.c_uint64(1)
    assert sx.lib().sx_print_findings_device(sc.h, res.h, 1, ord("x"), 0, C.byref(p), C.byref(n)) == sx.SX_E_STATE
    assert p.value is None and n.value == 0
    assert sx.OUTPUT_BOM + res.printed(radix="x") + b"\n" == want           # the caller then uses sx_print_findings
    res.free(); sc.close()
    # no findings at all
    sc = sx.Scanner(ms, device=0, result_on_device=True)
    res = sc.scan(bytes(1 << 20), file_id=1)
    assert len(res) == 0 and refused(res, radix="x") == sx.SX_E_STATE
    res.free(); sc.close()
    # the host merger
    monkeypatch.setenv("SX_HOST_MERGE", "1")
    sc = sx.Scanner(ms, device=0, result_on_device=True)
    res = sc.scan(data, file_id=1)
    assert refused(res, radix="x") == sx.SX_E_STATE
    assert sx.OUTPUT_BOM + res.printed(radix="x") + b"\n" == want
    res.free(); sc.close()


def test_a_segment_that_a_host_accessor_has_moved_is_refused(monkeypatch):
    monkeypatch.setenv("SX_MERGE_PART_FINDINGS", "7000")
    monkeypatch.setenv("SX_MERGE_PART_MIB", "1")
    ms, data, _ = case("A")
    sc = sx.Scanner(ms, device=0, result_on_device=True)
    try:
        res = sc.scan(data, file_id=1)
        assert len(res.device_segments()) >= 3
        text = device_text(sc, res, radix="x")
        fp, n, ap, alen = C.POINTER(sx.Finding)(), C.c_uint64(), C.POINTER(C.c_uint8)(), C.c_uint64()
        sc._chk(sx.lib().sx_result_segment(res.h, 1, C.byref(fp), C.byref(n), C.byref(ap), C.byref(alen)))   # segment 1 comes to the host
        assert refused(res, radix="x") == sx.SX_E_STATE
        assert res.printed(radix="x") == text
        res.free()
    finally:
        sc.close()


def test_a_later_scan_and_a_closed_scanner_are_refused():
    ms, data, _ = case("A")
    sc = sx.Scanner(ms, device=0, result_on_device=True)
    res = sc.scan(data, file_id=1)
    assert device_text(sc, res, radix="x")
    res2 = sc.scan(data[:4096 * 100], file_id=1)
    assert refused(res, radix="x") == sx.SX_E_STATE                 # a later scan has reused the memory
    assert device_text(sc, res2, radix="x") == res2.printed(radix="x")
    res3 = sc.scan(data[:4096 * 100], file_id=1)
    assert all(s[0] is not None for s in res3.device_segments())
    sc.close()                                                      # sx_destroy frees the result block and the text block
    with pytest.raises(sx.SxError):
        res3.printed_device(radix="x")
    with pytest.raises(sx.SxError):
        res3.device_segments()
    for r in (res, res2, res3):
        r.free()
    # a result of another Scanner: its memory is not this context's
    a, b = sx.Scanner(ms, device=0, result_on_device=True), sx.Scanner(ms, device=0, result_on_device=True)
    ra = a.scan(data[:4096 * 100], file_id=1)
    p, n = C.c_void_p(), C.c_uint64()
    assert sx.lib().sx_print_findings_device(b.h, ra.h, 1, ord("x"), 0, C.byref(p), C.byref(n)) == sx.SX_E_STATE
    ra.free(); a.close(); b.close()


def print_row(position, precision, s, completes, mission_id, labels):
    """Finding::print (src/finding.rs:112-155) with -t x, one input, several Missions"""
    return (b"\n" + {"After": b">", "Exact": b" ", "Before": b"<"}[precision] + b"%x" % position + (b"+\t" if completes else b" \t")
            + b"(" + bytes([mission_id + 97]) + b" " + labels[mission_id] + b")\t" + s.encode("utf-8"))


def test_config5_missions_on_4gib_of_background():
    """at scale: text_len against the line lengths computed from the downloaded records, and the oracle's rows of two sampled
    windows (as tests/test_gpu_result_on_device_multi.py samples them), formatted here, each as ONE contiguous piece of the text"""
    from test_gpu_baseline_configs import SEED
    from test_gpu_scale import MARGIN, WINDOW, oracle_window, regenerate
    ms = sx.missions_from_flags(**C5)
    assert [sx.encoding_name(m["encoding"]).encode() for m in ms] == [C5_LABELS[k] for k in range(6)]
    total = 4 << 30
    sc = sx.Scanner(ms, device=0, result_on_device=True)
    d = sc.alloc(total)
    try:
        sc.fill_background(d, 0, total, SEED)
        res = sc.scan_device(d, total, file_id=1)
        dsegs = res.device_segments()
        assert all(s[0] is not None for s in dsegs) and sum(s[1] for s in dsegs) == len(res) > 15_000_000
        p, text_len = res.printed_device(n_inputs=1, radix="x")
        assert pointers(res) == [(s[0], s[1], s[2], s[3], s[4]) for s in dsegs]
        # 1 + 1 + hex digits + 2 + 3 + label + 2 + str_len per line
        label_len = np.zeros(256, np.uint64)
        for k, v in C5_LABELS.items():
            label_len[k] = len(v)
        want_len, step = 0, 4 << 20
        for fp, n, ap, alen, packed, info in dsegs:
            assert packed
            for i0 in range(0, n, step):
                i1 = min(n, i0 + step)
                recs = np.frombuffer(sc.download(C.c_void_p(fp + i0 * 16), (i1 - i0) * 16), dtype=F16)
                pos = recs["position"]
                digits = np.ones(len(recs), np.uint64)
                for k in range(1, 16):
                    digits += pos >= np.uint64(16 ** k)
                want_len += int((digits + label_len[recs["mission_id"]] + recs["str_len"].astype(np.uint64)).sum()) + 9 * len(recs)
        assert text_len == want_len, (text_len, want_len)
        text = bytearray(text_len)
        piece = 256 << 20
        for o in range(0, text_len, piece):
            m = min(piece, text_len - o)
            sc._chk(sx.lib().sx_device_download(sc.h, (C.c_char * m).from_buffer(text, o), C.c_void_p(p + o), m))
        assert text[:1] == b"\n" and text.count(b"\n") >= len(res)
        rng = random.Random(2026)
        for ws in (total - WINDOW, rng.randrange(0, total - WINDOW) // 4096 * 4096):
            at_end = ws + WINDOW == total
            lo_slice, hi_slice = (ws + MARGIN) // 4096, (ws + WINDOW - (0 if at_end else MARGIN)) // 4096
            rows = [t for t in oracle_window(ms, regenerate(ws, WINDOW, []), ws) if lo_slice <= t[5] < hi_slice]
            assert len(rows) > 100_000
            expected = b"".join(print_row(t[0], t[1], t[2], t[3], t[4], C5_LABELS) for t in rows)
            assert expected in text, (hex(ws), len(rows))
            if at_end:
                assert text.endswith(expected)
        res.free()
    finally:
        sc.free(d); sc.close()
