"""The interleave of the Missions' findings (stringsext_amd/csrc/sx_sort.hip: merge_range_kernel, merge_bounds_kernel,
merge_place_kernel, the radix-sort fallback with merge_gather_in_kernel / merge_gather_out_kernel, merge_cuts_kernel, copy_bytes_kernel;
sx_merge.cpp drives them) on planted inputs (run with -m gpu on an MI355X), through Scanner.scan_device with device_replay=True.  The
plants are tests/record_plant.py's (test_record_plant.py pins what they rely on): lists that tie with a twin at every position, a
Mission with no findings, lists that lie apart, thousands of findings inside one tile of a position range one outlier stretches, totals
around one and two tiles, parts cut exactly where strings begin, more Missions than the one-pass merger takes, and the copy kernel at
every shape the switches give it.  The expected value is the oracle's text; where the result stays on the device its records are
compared one by one too.  Every case asserts from SX_TIMING's line that the device merged, of how many Missions and in how many parts."""
import pytest

import record_plant as rp
import refconfig as rc
import result_plant
import stringsext_amd as sx
from test_gpu_result_strides import check_records

pytestmark = pytest.mark.gpu

PLANTS = rp.interleave_plants()
PARTS = [("SX_MERGE_PART_FINDINGS", "1024"), ("SX_MERGE_PART_MIB", "1")]


def interleave(monkeypatch, capfd, flags, data, env=(), on_device=False, parts=False, what=""):
    """one Scanner (the switches are read when it is created), one scan_device call: the text == the oracle's, the device merged every
    list that has findings, in one part or (parts) in several; on_device: the records in HBM are the oracle's rows, in their order.
    -> (findings, parts, the Missions the device merged)"""
    monkeypatch.setenv("SX_TIMING", "1")
    for name, value in env:
        monkeypatch.setenv(name, value)
    ms = rc.missions(encodings=flags)
    rows = result_plant.expected(ms, data)
    with_findings = len(set(rows.mission.tolist()))
    sc = sx.Scanner(ms, device=0, device_replay=True, result_on_device=on_device)
    try:
        ptr = sc.alloc(len(data))
        sc.upload(ptr, data)
        capfd.readouterr()
        res = sc.scan_device(ptr, len(data), file_id=1)
        err = capfd.readouterr().err
        merges = rp.merge_lines(err)
        assert len(merges) == 1 and merges[0][:2] == (with_findings, rows.n), (what, merges, with_findings, rows.n, err[-2000:])
        n_parts, n_segments = merges[0][2], sx.lib().sx_result_segments(res.h)       # (a part with findings is a segment; reading one through the host's accessors would fetch it)
        if parts:
            assert n_parts > 1 and n_segments > 1, (what, merges, n_segments)
        else:
            assert n_parts == 1 and n_segments == 1, (what, merges, n_segments)
        if on_device:
            check_records(sc, res, rows, True, str(what))
        got = sx.OUTPUT_BOM + res.printed(n_inputs=1, radix="x") + b"\n"
        if got != rows.text():
            g, w = got.split(b"\n"), rows.text().split(b"\n")
            k = next((i for i in range(min(len(g), len(w))) if g[i] != w[i]), min(len(g), len(w)))
            raise AssertionError("%s: %d lines, %d wanted; first difference at finding %d: got %r, want %r"
                                 % (what, len(g), len(w), k - 1, g[k:k + 1], w[k:k + 1]))
        res.free()
        sc.free(ptr)
        return rows.n, n_parts, merges[0][0]
    finally:
        sc.close()


SHAPES = [(name, on_device) for name, p in PLANTS.items() if not name.startswith(("parts", "small_parts", "total"))
          for on_device in (False, True) if on_device or p.host_way]


@pytest.mark.parametrize("packed", ["1", "0"], ids=["packed", "unpacked"])
@pytest.mark.parametrize("name,on_device", SHAPES, ids=["%s-%s" % (n, "on_device" if d else "to_host") for n, d in SHAPES])
def test_lists_that_tie_lie_apart_or_are_empty(monkeypatch, capfd, name, on_device, packed):
    """twins at every position (merge_upper for the Missions in front, merge_lower for those behind), an empty list first, in the middle
    and last, a list wholly in front of and one wholly behind the others (bounds of 0 and of nf in every tile), thousands of findings in
    one tile of a range that one outlier stretches, in front or behind (merge_range_kernel's shift)"""
    p = PLANTS[name]
    interleave(monkeypatch, capfd, p.flags, p.data, env=[("SX_PACKED", packed)], on_device=on_device, what=(name, on_device, packed))


@pytest.mark.parametrize("packed", ["1", "0"], ids=["packed", "unpacked"])
@pytest.mark.parametrize("total", rp.INTERLEAVE_TOTALS)
def test_totals_around_one_and_two_tiles(monkeypatch, capfd, total, packed):
    """T = n / 64 tiles, one at least: 1 and 63 findings (n / 64 = 0) make the one tile, 64 and 65 make one, 129 two — n counts all four
    lists, a twin's among them; the result stays on the device"""
    p = PLANTS["total%d" % total]
    n, _, _ = interleave(monkeypatch, capfd, p.flags, p.data, env=[("SX_PACKED", packed)], on_device=True, what=("total", total, packed))
    assert n == total       # (rows.n, which interleave() found in the merge's timing line)


@pytest.mark.parametrize("on_device", [False, True], ids=["to_host", "on_device"])
@pytest.mark.parametrize("name", ["parts", "small_parts"])
def test_parts_cut_where_strings_begin(monkeypatch, capfd, name, on_device):
    """parts of at most 1024 findings: merge_cuts_kernel's cuts fall on strings that begin exactly at a slice boundary, behind the last
    finding of a list that ends in front of the first cut, and in front of and behind a list that lies inside one part (str_off counts
    from a non-zero off0 in every part but the first)"""
    p = PLANTS[name]
    _, n_parts, _ = interleave(monkeypatch, capfd, p.flags, p.data, env=PARTS, on_device=on_device, parts=True, what=(name, on_device))
    assert n_parts >= 8


@pytest.mark.parametrize("parts", [False, True], ids=["one_part", "parts"])
@pytest.mark.parametrize("n", [17, 18, 26])
def test_more_missions_than_the_one_pass_merger_takes(monkeypatch, capfd, n, parts):
    """17, 18 and 26 Missions: the stable radix sort over the concatenation — ties between Missions on either side of the 16th keep
    the Missions' order, a Mission without findings among them, merge_gather_in_kernel's string offsets with a non-zero off0 (parts)"""
    lists = rp.constant("kMergeLists")
    assert lists == 16 and n > lists
    flags = rp.many_missions(n)
    _, _, merged = interleave(monkeypatch, capfd, flags, rp.many_plant(), env=PARTS if parts else [], parts=parts, what=(n, parts))
    assert merged == (n if n == lists + 1 else n - 1)       # (the timing line's "device merge of 17 missions"; beyond 17 one Mission finds nothing)


_copy_plants = {}
COPY_SHAPES = [(wgs, threads, nt) for wgs in ("1", "2", "3", "64") for threads in ("64", "1024") for nt in ("0", "1")]


@pytest.mark.parametrize("wgs,threads,nt", COPY_SHAPES, ids=["wgs%s-t%s-nt%s" % c for c in COPY_SHAPES])
def test_copy_kernel_shapes(monkeypatch, capfd, wgs, threads, nt):
    """a part of more than 1 MiB whose byte count is 0, 1 and 15 modulo 16 (copy_bytes_kernel's tail of up to 15 bytes), copied by 1,
    2, 3 and 64 workgroups of 64 and 1024 threads: stretches of many trips of the four-deep loop, of none (64 x 1024: a stretch is
    shorter than four strides), and the loop's boundary in between; stores non-temporal or not"""
    env = [("SX_MERGE_COPY_WGS", wgs), ("SX_MERGE_COPY_THREADS", threads), ("SX_MERGE_COPY_NT", nt)]
    flags = [rp.mission_flag("ascii"), rp.mission_flag("Cyrillic")]
    for residue in rp.COPY_RESIDUES:
        if residue not in _copy_plants:
            _copy_plants[residue] = rp.copy_plant(residue)
        interleave(monkeypatch, capfd, flags, _copy_plants[residue], env=env, what=("copy", wgs, threads, nt, residue))


@pytest.mark.parametrize("wgs,threads", [("64", "64"), ("3", "1024")])
def test_copy_kernel_small_parts(monkeypatch, capfd, wgs, threads):
    """parts of a few findings: fewer 16-byte words than four strides, and (64 workgroups) workgroups whose stretch is empty"""
    p = PLANTS["small_parts"]
    env = PARTS + [("SX_MERGE_COPY_WGS", wgs), ("SX_MERGE_COPY_THREADS", threads)]
    interleave(monkeypatch, capfd, p.flags, p.data, env=env, parts=True, what=("small parts", wgs, threads))
