"""SX_OPT_RESULT_ON_DEVICE with several Missions (include/stringsext_amd.h): the merged findings stay in HBM, one segment per
merger part, records as the merger writes them (sx_finding16 where it can pack), the strings of a segment back to back in record
order.  Every case is compared with the oracle's text and with a Scanner without the flag; the cases in which the result stays in
host memory (the header's list) must give a correct host result."""
import ctypes as C
import random

import numpy as np
import pytest

import refconfig as rc
import stringsext_amd as sx
import sxo_binding as sxo
from test_host_logic import synth
from test_wave_core import text_lines

pytestmark = pytest.mark.gpu

F16 = np.dtype({"names": ["position", "str_off", "str_len", "flags", "mission_id"], "formats": ["<u8", "<u4", "<u2", "u1", "u1"],
                "offsets": [0, 8, 12, 14, 15], "itemsize": 16})
F32 = np.dtype({"names": ["position", "str_off", "str_len", "precision", "completes", "mission_id", "file_id", "slice_index"],
                "formats": ["<u8", "<u4", "<u4", "u1", "u1", "u1", "<i2", "<u4"], "offsets": [0, 8, 12, 16, 17, 18, 20, 24], "itemsize": 32})
C5 = dict(encodings=["utf-8,,,African", "utf-16le,,,African", "utf-16be,,,African", "big5,,,Cjk", "euc-jp,,,Asian", "koi8-r,,,Cyrillic"],
          chars_min="10")


def input_a():
    rng = random.Random(2026)
    return (text_lines(rng, 1_500_000) + text_lines(rng, 600_000).decode().encode("utf-16-le") + rng.randbytes(1_000_000)
            + text_lines(rng, 300_000).decode().encode("utf-16-be"))


def case(name):
    """(Missions, input, the Missions the oracle must report findings for)"""
    rng = random.Random(2026)
    if name == "A":   # dense, four Missions
        return rc.missions(encodings=["ascii", "utf-8", "utf-16le", "utf-16be"], chars_min="5"), input_a(), "abcd"
    if name == "B":   # BASELINE config 5's Missions on random bytes: two of the six stay empty
        return sx.missions_from_flags(**C5), rng.randbytes(8 << 20), "adef"
    if name == "C":   # sparse: the lane-per-region replay (or, replayed on the host, the upload)
        return rc.missions(encodings=["utf-8", "utf-16le"], chars_min="10"), synth(rng, 4_000_000, 1 / 400), "ab"
    if name == "D":   # one Mission with findings among two
        return rc.missions(encodings=["ascii", "utf-16le,,,African"], chars_min="40"), text_lines(rng, 1_000_000), "a"
    raise KeyError(name)


def oracle_text(ms, data, letters):
    want = sxo.run_cli(ms, [data], radix="x")
    for c in letters:   # (the case cannot pass empty)
        assert b"(%c " % c.encode() in want, c
    return want


def framed(res):
    return sx.OUTPUT_BOM + res.printed(n_inputs=1, radix="x") + b"\n"


def download_segment(sc, seg):
    """(records as a numpy array, strings) of one device segment; checks the layout rule"""
    fp, n, ap, alen, packed, info = seg
    assert fp is not None and n > 0
    recs = np.frombuffer(sc.download(fp, n * (16 if packed else 32)), dtype=F16 if packed else F32)
    arena = sc.download(ap, alen) if alen else b""
    off, ln = recs["str_off"].astype(np.uint64), recs["str_len"].astype(np.uint64)
    assert off[0] == 0 and np.array_equal(off[1:], (off + ln)[:-1]) and int((off + ln)[-1]) == alen == int(ln.sum())   # back to back, in record order
    return recs, arena


def expanded(recs, arena, packed, info):
    """what the host accessors make of the records: dicts as Result.findings() returns them"""
    out = []
    for r in recs:
        o, n, mid, pos = int(r["str_off"]), int(r["str_len"]), int(r["mission_id"]), int(r["position"])
        if packed:
            prec, comp, fid = int(r["flags"]) & 3, bool(int(r["flags"]) & 4), info.input_file_id
            sl = info.slice_base + (pos - info.position0[mid]) // 4096
        else:
            prec, comp, fid, sl = int(r["precision"]), bool(r["completes"]), int(r["file_id"]), int(r["slice_index"])
        out.append(dict(position=pos, precision=sx.PRECISION[prec], s=arena[o:o + n].decode("utf-8"), completes=comp, mission_id=mid,
                        file_id=fid, slice_index=sl))
    return out


def check_on_device(ms, data, letters, device_replay=None, packed=True, min_segments=1):
    want = oracle_text(ms, data, letters)
    ref = sx.Scanner(ms, device=0, device_replay=device_replay)
    host = ref.scan(data, file_id=1)
    sc = sx.Scanner(ms, device=0, device_replay=device_replay, result_on_device=True)
    try:
        res = sc.scan(data, file_id=1)
        dsegs = res.device_segments()
        assert len(dsegs) >= min_segments and all(s[0] is not None for s in dsegs), [(s[0], s[1]) for s in dsegs]   # all of it in HBM
        assert all(s[4] == packed for s in dsegs)
        got = []
        for seg in dsegs:
            recs, arena = download_segment(sc, seg)
            got += expanded(recs, arena, seg[4], seg[5])
        host_f = host.findings()
        assert len(got) == len(host_f) == len(res)
        assert got == host_f, next((a, b) for a, b in zip(got, host_f) if a != b)
        assert framed(host) == want
        assert framed(res) == want                                                   # the host accessors fetch on first use ...
        assert all(s[0] is None for s in res.device_segments())                      # ... and then it lies in host memory
        assert res.findings() == host_f
        res2 = sc.scan(data, file_id=1)                                              # (carried state: the second buffer of a stream)
        assert all(s[0] is not None for s in res2.device_segments())
        res3 = sc.scan(data[:4096 * 10], file_id=1)
        with pytest.raises(sx.SxError):
            res2.device_segments()
        with pytest.raises(sx.SxError):
            res2.segments()
        for r in (res, res2, res3):
            r.free()
        return len(dsegs)
    finally:
        sc.close(); host.free(); ref.close()


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_several_missions_result_stays_on_the_device(name):
    ms, data, letters = case(name)
    check_on_device(ms, data, letters)


def test_lists_replayed_on_the_host_are_uploaded():
    """few runs / SX_OPT_HOST_REPLAY: the Missions' findings exist on the host only and join the merge through the upload"""
    ms, data, letters = case("C")
    check_on_device(ms, data, letters, device_replay=False, packed=True)


def test_iso2022jp_next_to_utf8_is_on_the_device():
    """ISO-2022-JP's one sequential pass runs on the host: its list is uploaded, the result is on the device all the same"""
    from test_iso2022jp import soup
    rng = random.Random(2026)
    data = soup(rng, 400_000) + rng.randbytes(300_000) + text_lines(rng, 200_000) + soup(rng, 100_000)
    ms = rc.missions(encodings=["utf-8", "iso-2022-jp"], chars_min="5", unicode_block_filter="All")
    check_on_device(ms, data, "ab")


def test_unpacked_records_have_the_same_layout(monkeypatch):
    monkeypatch.setenv("SX_PACKED", "0")
    ms, data, letters = case("A")
    check_on_device(ms, data, letters, packed=False)


def test_several_parts_are_several_device_segments(monkeypatch):
    """every part has its own str_off space; a part fetched by a host accessor leaves the others' pointers alone"""
    monkeypatch.setenv("SX_MERGE_PART_FINDINGS", "7000")
    monkeypatch.setenv("SX_MERGE_PART_MIB", "1")
    ms, data, letters = case("A")
    assert check_on_device(ms, data, letters, min_segments=2) >= 2
    ref = sx.Scanner(ms, device=0)
    host = ref.scan(data, file_id=1)
    sc = sx.Scanner(ms, device=0, result_on_device=True)
    try:
        res = sc.scan(data, file_id=1)
        before = res.device_segments()
        assert len(before) >= 3 and all(s[0] is not None and s[0] % 256 == 0 for s in before)
        fp, n, ap, alen = C.POINTER(sx.Finding)(), C.c_uint64(), C.POINTER(C.c_uint8)(), C.c_uint64()
        sc._chk(sx.lib().sx_result_segment(res.h, 1, C.byref(fp), C.byref(n), C.byref(ap), C.byref(alen)))   # segment 1 comes to the host
        after = res.device_segments()
        assert after[1][0] is None and all(s[0] is not None for i, s in enumerate(after) if i != 1)
        assert [(s[0], s[1], s[2], s[3]) for i, s in enumerate(after) if i != 1] == [(s[0], s[1], s[2], s[3]) for i, s in enumerate(before) if i != 1]
        got = []
        for i, seg in enumerate(after):
            if i == 1:
                arena = C.string_at(ap, alen.value)
                got += [dict(position=fp[j].position, precision=sx.PRECISION[fp[j].precision], s=arena[fp[j].str_off:fp[j].str_off + fp[j].str_len].decode("utf-8"),
                             completes=bool(fp[j].completes_previous), mission_id=fp[j].mission_id, file_id=fp[j].input_file_id,
                             slice_index=fp[j].slice_index) for j in range(n.value)]
            else:
                recs, arena = download_segment(sc, seg)
                got += expanded(recs, arena, seg[4], seg[5])
        assert got == host.findings()
        res.free()
    finally:
        sc.close(); host.free(); ref.close()


def test_carried_state_over_two_scans():
    ms, data, letters = case("A")
    want = oracle_text(ms, data, letters)
    cut = (len(data) // 2) // 4096 * 4096 + 4096
    sc = sx.Scanner(ms, device=0, result_on_device=True)
    try:
        out = bytearray(sx.OUTPUT_BOM)
        for chunk in (data[:cut], data[cut:]):
            res = sc.scan(chunk, file_id=1)
            dsegs = res.device_segments()
            assert dsegs and all(s[0] is not None for s in dsegs)
            for seg in dsegs:
                download_segment(sc, seg)
            out += res.printed(n_inputs=1, radix="x")
            res.free()
        assert bytes(out) + b"\n" == want
    finally:
        sc.close()


def host_result_is_right(ms, data, letters, want=None):
    want = want if want is not None else oracle_text(ms, data, letters)
    sc = sx.Scanner(ms, device=0, result_on_device=True)
    try:
        res = sc.scan(data, file_id=1)
        assert all(s[0] is None for s in res.device_segments())      # all or nothing: here nothing
        assert framed(res) == want
        res.free()
    finally:
        sc.close()


@pytest.mark.parametrize("env", [{"SX_SEQ_PIECE_KIB": "512"}, {"SX_HOST_MERGE": "1"}, {"SX_PIECE_MIB": "1"}])
def test_forced_pieces_and_the_host_merger_give_a_host_result(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ms, data, letters = case("A")
    host_result_is_right(ms, data, letters)


def test_missions_that_count_from_different_origins_give_a_host_result():
    ms, data, letters = case("A")
    ms = [dict(m, counter_offset=1000 * k) for k, m in enumerate(ms)]   # (by hand: the front end gives all Missions the same -s)
    host_result_is_right(ms, data, letters)


def test_no_findings_at_all_gives_a_host_result():
    ms, _, _ = case("A")
    data = bytes(1 << 20)
    host_result_is_right(ms, data, "", want=sxo.run_cli(ms, [data], radix="x"))


def test_scan_file_in_chunks(tmp_path):
    """as tests/test_gpu_wave.py describes it for one Mission: the last chunk's result is on the device; an earlier one is either
    refused (a later chunk has reused the block) or was moved to the host in time, and then it is right"""
    ms, data, _ = case("A")
    data = data[:3 * (1 << 20) + 12345]
    path = tmp_path / "in.bin"
    path.write_bytes(data)
    ref = sx.Scanner(ms, device=0)
    want = [r for r in ref.scan_file(str(path), chunk_bytes=1 << 20)]
    sc = sx.Scanner(ms, device=0, result_on_device=True)
    got = sc.scan_file(str(path), chunk_bytes=1 << 20)
    assert len(got) == len(want) >= 3
    assert all(s[0] is not None for s in got[-1].device_segments())
    assert got[-1].findings() == want[-1].findings()
    for r, w in zip(got[:-1], want[:-1]):
        try:
            segs = r.device_segments()
        except sx.SxError:
            continue
        assert all(s[0] is None for s in segs)
        assert r.findings() == w.findings()
    last = sc.scan(data[:1 << 20], file_id=1)
    assert last.device_segments()[0][0] is not None
    sc.close()
    with pytest.raises(sx.SxError):
        last.device_segments()
    for r in want:
        r.free()
    ref.close()


def test_config5_missions_on_4gib_of_background():
    """at scale: by count against a Scanner without the flag, the layout rule over all records (downloaded in slices), and the
    oracle's text on sampled windows as tests/test_gpu_scale.py samples them"""
    from test_gpu_baseline_configs import SEED
    from test_gpu_scale import MARGIN, WINDOW, oracle_window, regenerate
    ms = sx.missions_from_flags(**C5)
    total = 4 << 30
    ref = sx.Scanner(ms, device=0)
    d = ref.alloc(total)
    ref.fill_background(d, 0, total, SEED)
    host = ref.scan_device(d, total, file_id=1)
    n_host = len(host)
    host.free()
    sc = sx.Scanner(ms, device=0, result_on_device=True)
    try:
        res = sc.scan_device(d, total, file_id=1)
        dsegs = res.device_segments()
        assert all(s[0] is not None for s in dsegs) and sum(s[1] for s in dsegs) == len(res) == n_host > 15_000_000
        rng = random.Random(2026)
        starts = [total - WINDOW, rng.randrange(0, total - WINDOW) // 4096 * 4096]
        wanted = []
        for ws in starts:
            at_end = ws + WINDOW == total
            lo_slice, hi_slice = (ws + MARGIN) // 4096, (ws + WINDOW - (0 if at_end else MARGIN)) // 4096
            wanted.append((ws, lo_slice, hi_slice, []))
        step = 4 << 20   # records per download
        for fp, n, ap, alen, packed, info in dsegs:
            assert packed
            pos0 = np.array(info.position0[:256], dtype=np.uint64)
            end_prev = 0
            for i0 in range(0, n, step):
                i1 = min(n, i0 + step)
                recs = np.frombuffer(sc.download(C.c_void_p(fp + i0 * 16), (i1 - i0) * 16), dtype=F16)
                off, ln = recs["str_off"].astype(np.uint64), recs["str_len"].astype(np.uint64)
                assert int(off[0]) == end_prev and np.array_equal(off[1:], (off + ln)[:-1])
                end_prev = int(off[-1] + ln[-1])
                sl = info.slice_base + (recs["position"] - pos0[recs["mission_id"]]) // 4096
                assert np.all(sl[1:] >= sl[:-1])                                       # print order: slice by slice
                for ws, lo_slice, hi_slice, rows in wanted:
                    j0, j1 = np.searchsorted(sl, [lo_slice, hi_slice])
                    if j1 > j0:
                        a0, a1 = int(off[j0]), int(off[j1 - 1] + ln[j1 - 1])
                        arena = sc.download(C.c_void_p(ap + a0), a1 - a0)
                        for r, s in zip(recs[j0:j1], sl[j0:j1]):
                            o = int(r["str_off"]) - a0
                            rows.append((int(r["position"]), sx.PRECISION[int(r["flags"]) & 3], arena[o:o + int(r["str_len"])].decode("utf-8"),
                                         bool(int(r["flags"]) & 4), int(r["mission_id"]), int(s)))
            assert end_prev == alen
        for ws, lo_slice, hi_slice, rows in wanted:
            want = [t for t in oracle_window(ms, regenerate(ws, WINDOW, []), ws) if lo_slice <= t[5] < hi_slice]
            assert len(want) > 100_000
            assert rows == want, (hex(ws), len(rows), len(want), next(((a, b) for a, b in zip(rows, want) if a != b), None))
        res.free()
    finally:
        sc.close(); ref.free(d); ref.close()
