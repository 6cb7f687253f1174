"""The ordered string gather of a merged part that stays in HBM (stringsext_amd/csrc/sx_result_core.hpp: SX_OPT_RESULT_ON_DEVICE
with several Missions), compiled as plain host C++ and driven the way sx_sort.hip / sx_result_dev.hip drive it (tests/native/
result_core_host.cpp: placement by rank, a scan over str_len, then wavefront after wavefront the core's two lane loops), against a
plain Python merge of seeded lists: record order (position, then Mission), the layout rule of include/stringsext_amd.h — the strings
back to back in record order — and the string bytes."""
import ctypes as C
import os
import random
import subprocess

import pytest

import stringsext_amd as sx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "stringsext_amd", "csrc")


def build_result_core():
    """(as tests/native/build_harness.py builds the other cores: g++ on one file, rebuilt when a source is newer)"""
    so, src = os.path.join(NATIVE, "libresult_core_host.so"), os.path.join(NATIVE, "result_core_host.cpp")
    deps = [src, os.path.join(CSRC, "sx_result_core.hpp"), os.path.join(ROOT, "include", "stringsext_amd.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in deps):
        tmp = f"{so}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", tmp, src])
        os.replace(tmp, so)
    return so


@pytest.fixture(scope="module")
def core():
    L = C.CDLL(build_result_core())
    L.sxr_merge_ordered_host.restype = C.c_int
    L.sxr_merge_ordered_host.argtypes = [C.c_int, C.POINTER(C.POINTER(sx.Finding)), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint32), C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    return L


def make_list(rng, mission_id, n, positions=None, off0=0, lens=None):
    """a Mission's findings as stage B leaves them: ordered by position, strings in the same order; str_off counts from a
    point `off0` bytes in front of the part's first string (the merger cuts a list into parts)"""
    pos = sorted(positions if positions is not None else (rng.randrange(0, 1 << 20) for _ in range(n)))
    recs, arena = [], bytearray()
    for i, p in enumerate(pos):
        ln = lens[i] if lens is not None else rng.choice((0, 1, 3, 5, 15, 16, 17, 31, 64, 200)) if rng.random() < 0.3 else rng.randrange(4, 24)
        s = bytes(rng.randrange(1, 256) for _ in range(ln))
        recs.append(dict(position=p, str_off=off0 + len(arena), str_len=ln, precision=rng.randrange(3), completes=rng.randrange(2),
                         mission_id=mission_id, file_id=3, slice_index=p // 4096, s=s))
        arena += s
    return recs, bytes(arena), off0


def python_merge(lists):
    """the merger's order (src/main.rs:118-136): by position, ties by Mission; stable within a list"""
    out = []
    for m, (recs, _, _) in enumerate(lists):
        out += [(r["position"], m, i, r) for i, r in enumerate(recs)]
    out.sort(key=lambda t: t[:3])
    return [t[3] for t in out]


def run_core(L, lists, packed, misalign=0):
    nm = len(lists)
    keep = []
    fps = (C.POINTER(sx.Finding) * nm)()
    aps = (C.c_void_p * nm)()
    nfs = (C.c_uint64 * nm)()
    off0 = (C.c_uint32 * nm)()
    for m, (recs, arena, o0) in enumerate(lists):
        arr = (sx.Finding * max(1, len(recs)))()
        for i, r in enumerate(recs):
            arr[i] = sx.Finding(r["position"], r["str_off"], r["str_len"], r["precision"], r["completes"], r["mission_id"], 0, r["file_id"], 0,
                                r["slice_index"])
        buf = C.create_string_buffer(arena, max(1, len(arena)))
        keep += [arr, buf]
        fps[m] = C.cast(arr, C.POINTER(sx.Finding)); aps[m] = C.addressof(buf); nfs[m] = len(recs); off0[m] = o0
    n = sum(len(x[0]) for x in lists)
    total = sum(len(x[1]) for x in lists)
    Rec = sx.Finding16 if packed else sx.Finding
    out = (Rec * max(1, n))()
    raw = C.create_string_buffer(b"\xEE" * (total + 64 + 16), total + 64 + 16)
    base = C.addressof(raw)
    base += (-base) % 16 + misalign   # (the product's arenas are 16-byte aligned; the core must not rely on it)
    alen = C.c_uint64()
    rcode = L.sxr_merge_ordered_host(nm, fps, aps, nfs, off0, int(packed), out, base, total, C.byref(alen))
    assert rcode == 0, rcode
    arena = C.string_at(base, total + 32)
    assert alen.value == total
    assert arena[total:] == b"\xEE" * 32, "bytes behind the arena were written"
    assert C.string_at(C.addressof(raw), base - C.addressof(raw)) == b"\xEE" * (base - C.addressof(raw)), "bytes in front of the arena were written"
    return out, arena[:total]


def check(L, lists, packed, misalign=0):
    want = python_merge(lists)
    out, arena = run_core(L, lists, packed, misalign)
    assert len(arena) == sum(r["str_len"] for r in want)          # arena_len == sum(str_len)
    off = 0
    for i, r in enumerate(want):
        g = out[i]
        assert g.position == r["position"] and g.mission_id == r["mission_id"], (i, g.position, r["position"])
        assert g.str_off == off and g.str_len == r["str_len"], (i, g.str_off, off)   # str_off[0] == 0, str_off[i + 1] == str_off[i] + str_len[i]
        assert arena[off:off + g.str_len] == r["s"], i
        if packed:
            assert g.flags == (r["precision"] | (4 if r["completes"] else 0))
        else:
            assert (g.precision, g.completes_previous, g.input_file_id, g.slice_index) == (r["precision"], r["completes"], r["file_id"], r["slice_index"])
        off += g.str_len


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("nm", [2, 3, 6, 16])
def test_seeded_lists(core, nm, packed):
    rng = random.Random(1000 + nm)
    for sizes in ([rng.randrange(1, 400) for _ in range(nm)], [rng.randrange(0, 70) for _ in range(nm)], [1000] + [3] * (nm - 1)):
        check(core, [make_list(rng, m, sizes[m]) for m in range(nm)], packed)


@pytest.mark.parametrize("packed", [True, False])
def test_empty_lists_and_a_single_list_with_findings(core, packed):
    rng = random.Random(7)
    check(core, [make_list(rng, 0, 0), make_list(rng, 1, 130), make_list(rng, 2, 0)], packed)
    check(core, [make_list(rng, 0, 64), make_list(rng, 1, 0)], packed)     # exactly one wavefront's records
    check(core, [make_list(rng, 0, 0), make_list(rng, 1, 1)], packed)
    check(core, [make_list(rng, 0, 0), make_list(rng, 1, 0)], packed)      # nothing at all


@pytest.mark.parametrize("packed", [True, False])
def test_equal_positions_are_ordered_by_mission(core, packed):
    rng = random.Random(8)
    pos = [4096 * (i // 3) for i in range(300)]   # three findings per position in every list, the same positions in all of them
    lists = [make_list(rng, m, 0, positions=pos) for m in range(4)]
    want = python_merge(lists)
    assert [r["mission_id"] for r in want[:12]] == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3
    check(core, lists, packed)


@pytest.mark.parametrize("packed", [True, False])
def test_zero_length_strings(core, packed):
    rng = random.Random(9)
    lens = [0 if i % 3 else rng.randrange(1, 40) for i in range(200)]
    check(core, [make_list(rng, 0, 200, lens=lens), make_list(rng, 1, 200, lens=[0] * 200), make_list(rng, 2, 70, lens=[0] * 69 + [5])], packed)


@pytest.mark.parametrize("packed", [True, False])
def test_a_string_of_16000_bytes(core, packed):
    rng = random.Random(10)
    lens = [rng.randrange(4, 24) for _ in range(150)]
    lens[40] = 16000
    lens[41] = 16000
    lens[149] = 16000
    check(core, [make_list(rng, 0, 150, lens=lens), make_list(rng, 1, 90)], packed)


@pytest.mark.parametrize("packed", [True, False])
def test_a_part_whose_strings_start_at_a_nonzero_offset(core, packed):
    rng = random.Random(11)
    check(core, [make_list(rng, 0, 100, off0=123457), make_list(rng, 1, 77, off0=0xFFFF0000), make_list(rng, 2, 5, off0=1)], packed)


@pytest.mark.parametrize("misalign", [1, 7, 15])
def test_an_arena_that_is_not_16_byte_aligned(core, misalign):
    rng = random.Random(12 + misalign)
    check(core, [make_list(rng, 0, 300), make_list(rng, 1, 200)], True, misalign)
