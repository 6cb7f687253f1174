"""The findings of a device-resident result in sorted order (sx_result_order_device): the lane functions (stringsext_amd/csrc/
sx_order_core.hpp) compiled as plain host C++ and driven the way sx_order_dev.hip and the entry point drive them
(tests/native/order_core_host.cpp: pick, the scan, number; per round word, three stable sorts, split, the scan, compact; measure and
gather), against Python's sorted() over the strings.  No expected value comes from the code under test.  Every segment's arena ends
where a page without access begins: the core may read nothing behind the last string.

The model's numbers.  The order is sorted(range(n), key, reverse) over the findings that take part.  Round d looks at the bytes
[8d, 8d + 8) of the strings still undecided; a finding is decided in round min over its neighbours in sorted order of lcp // 8, where
lcp is the longest common prefix with a neighbour (an equal string: its own length): a group of one is decided, and a group whose
strings ended inside the word is.  rounds = 1 + the largest such number, max_depth = rounds - 1; tied = the kept findings whose key
equals a kept neighbour's."""
import ctypes as C
import os
import random
import subprocess

import pytest

import stringsext_amd as sx
from test_select_core import lay_out, records, text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "stringsext_amd", "csrc")
DEPS = [os.path.join(ROOT, "include", "stringsext_amd.h"), os.path.join(NATIVE, "seen_set_host.hpp"), os.path.join(NATIVE, "guarded_host.hpp"), os.path.join(NATIVE, "order_core_host.cpp")] + [
    os.path.join(CSRC, f) for f in ("sx_order_core.hpp", "sx_label_core.hpp", "sx_seen_core.hpp", "sx_distinct_core.hpp", "sx_select_core.hpp", "sx_seltally_core.hpp")]
STRING, FIELD, DESC, NOCASE = sx.SX_ORDER_BY_STRING, sx.SX_ORDER_BY_LABEL_FIELD, sx.SX_ORDER_DESCENDING, sx.SX_ORDER_NOCASE
POS0 = {m: 4096 * (m + 1) for m in range(5)}        # a packed segment's position0 by mission_id (records(): mission_id = i % 5)
FILE_ID, SLICE_BASE = 6, 11


def built(out, flags):
    out, src = os.path.join(NATIVE, out), os.path.join(NATIVE, "order_core_host.cpp")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in DEPS):
        tmp = f"{out}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + ["-o", tmp, src])
        os.replace(tmp, out)
    return out


@pytest.fixture(scope="module")
def core():
    L = C.CDLL(built("liborder_core_host.so", ["-O2", "-fPIC", "-shared"]))
    u64p, u32p, vpp = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_void_p)
    L.sxs_order_host.restype = C.c_int
    L.sxs_order_host.argtypes = [C.c_uint32, vpp, vpp, u64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), u32p, vpp, vpp, u32p, u64p, C.c_uint32,
                                 u64p, u64p, C.c_uint32, u64p, C.c_void_p, C.c_void_p]
    L.sxs_order_word.restype = None
    L.sxs_order_word.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u64p, u32p]
    L.sxs_guarded.restype, L.sxs_guarded.argtypes = C.c_void_p, [C.c_uint64, C.POINTER(C.c_void_p), u64p]
    L.sxs_unmap.restype, L.sxs_unmap.argtypes = None, [C.c_void_p, C.c_uint64]
    return L


def fold(s):
    """'A'..'Z' as 'a'..'z', no other byte"""
    return bytes(b | 0x20 if 0x41 <= b <= 0x5A else b for b in s)


def picked(label, any_, all_, none):
    return (any_ == 0 or label & any_ != 0) and label & all_ == all_ and label & none == 0


def lcp(a, b):
    n = 0
    while n < len(a) and n < len(b) and a[n] == b[n]:
        n += 1
    return n


def model(keys, descending, limit, by_string):
    """(the order as indices into `keys`, info) — `keys`: the (folded) strings or the fields of the findings that take part"""
    order = sorted(range(len(keys)), key=lambda i: keys[i], reverse=descending)
    kept = min(limit, len(keys)) if limit else len(keys)
    rounds = 0
    if by_string and keys:
        ks = [keys[i] for i in order]
        rounds = 1 + max(max(lcp(ks[p], ks[p - 1]) if p else 0, lcp(ks[p], ks[p + 1]) if p + 1 < len(ks) else 0) // 8 for p in range(len(ks)))
    k = [keys[i] for i in order[:kept]]
    tied = sum(1 for p in range(kept) if (p and k[p - 1] == k[p]) or (p + 1 < kept and k[p + 1] == k[p]))
    return order, dict(findings=len(keys), kept=kept, rounds=rounds, tied=tied, max_depth=max(rounds - 1, 0))


def expanded(rec, packed, s):
    """what sx_result_segment() gives for a record of records(): every field but str_off"""
    if not packed:
        return (rec.position, len(s), rec.precision, rec.completes_previous, rec.mission_id, rec.input_file_id, rec.slice_index)
    return (rec.position, len(s), rec.flags & 3, rec.flags >> 2 & 1, rec.mission_id, FILE_ID, SLICE_BASE + (rec.position - POS0[rec.mission_id]) // 4096 & 0xFFFFFFFF)


def run(L, segments, labels=None, by=STRING, flags=0, shift=0, bits=64, any_=0, all_=0, none=0, limit=0, packed=True, layout="packed", groups=2, rng=None):
    """the harness over `segments` (lists of strings) and `labels` (a list of words per segment, or None); returns (the keys of the
    whole order as (segment, record), the written records as (fields, string), info, the undecided slots after each round)"""
    rng = rng or random.Random(len(segments))
    n_segs, total = len(segments), sum(len(s) for s in segments)
    packed = [packed] * n_segs if isinstance(packed, bool) else list(packed)
    regions, keep = [], []
    vp = C.c_void_p * n_segs
    recs, arenas, pos0s, labs = vp(), vp(), vp(), vp()
    ns, pk, fid, sb = (C.c_uint64 * n_segs)(), (C.c_int32 * n_segs)(), (C.c_int32 * n_segs)(), (C.c_uint32 * n_segs)()
    pos0 = (C.c_uint64 * 256)(*[POS0.get(m, 0) for m in range(256)])
    try:
        for s, strings in enumerate(segments):
            offs, arena = lay_out(strings, layout, rng)
            region, region_bytes = C.c_void_p(), C.c_uint64()
            base = L.sxs_guarded(max(1, len(arena)), C.byref(region), C.byref(region_bytes))
            assert base
            regions.append((region, region_bytes))
            C.memmove(base, arena, len(arena))
            arr = records(strings, offs, packed[s])
            if packed[s]:
                for i in range(len(strings)):
                    arr[i].position += 4096 * 8      # (behind every position0)
            lab = (C.c_uint64 * max(1, len(strings)))(*(labels[s] if labels else []))
            keep += [arr, lab]
            recs[s], arenas[s], ns[s], pk[s] = C.addressof(arr), base, len(strings), int(packed[s])
            fid[s], sb[s], pos0s[s], labs[s] = (FILE_ID, SLICE_BASE, C.addressof(pos0), C.addressof(lab)) if packed[s] else (-1, 0, None, C.addressof(lab))
        info, left = (C.c_uint64 * 5)(), (C.c_uint64 * 4096)()
        order = (C.c_uint64 * (total + 1))()
        out = (sx.Finding * (total + 1))()
        out_arena = C.create_string_buffer(sum(len(x) for s in segments for x in s) + 1)
        spec, masks = (C.c_uint32 * 4)(by, flags, shift, bits), (C.c_uint64 * 4)(any_, all_, none, limit)
        rc = L.sxs_order_host(n_segs, recs, arenas, ns, pk, fid, sb, pos0s, labs if labels else None, spec, masks, groups, info, left, 4096, order, out, out_arena)
        assert rc == 0, rc
        info = dict(findings=info[0], kept=info[1], rounds=info[2], tied=info[3], max_depth=info[4])
        keys = [(order[p] >> 32, order[p] & 0xFFFFFFFF) for p in range(info["findings"])]
        written = []
        for p in range(info["kept"]):
            f = out[p]
            written.append(((f.position, f.str_len, f.precision, f.completes_previous, f.mission_id, f.input_file_id, f.slice_index), f.str_off,
                            out_arena.raw[f.str_off:f.str_off + f.str_len]))
        sources = {(s, i): keep[2 * s][i] for s in range(n_segs) for i in range(len(segments[s]))}
        return keys, written, info, list(left)[:min(info["rounds"], 4096)], sources
    finally:
        for region, region_bytes in regions:
            L.sxs_unmap(region, region_bytes)


def check(L, segments, labels=None, by=STRING, flags=0, shift=0, bits=64, any_=0, all_=0, none=0, limit=0, every=True, want_rounds=None):
    """`segments` in packed, unpacked and mixed records, both layouts and two grids, against the model"""
    flat = [(s, i) for s, seg in enumerate(segments) for i in range(len(seg))]
    part = [(s, i) for s, i in flat if not (any_ or all_ or none) or picked(labels[s][i], any_, all_, none)]
    if by == STRING:
        keys = [fold(segments[s][i]) if flags & NOCASE else segments[s][i] for s, i in part]
    else:
        keys = [labels[s][i] >> shift & (1 << bits) - 1 for s, i in part]
    order, want_info = model(keys, bool(flags & DESC), limit, by == STRING)
    want_keys = [part[i] for i in order]
    mixed = [k % 2 == 0 for k in range(len(segments))]
    first = None
    for packed, layout in (((True, "packed"), (False, "scattered"), (mixed, "scattered"), (False, "packed")) if every else ((mixed, "packed"),)):
        for groups in (1, 3):
            keys_got, written, info, left, sources = run(L, segments, labels, by, flags, shift, bits, any_, all_, none, limit, packed, layout, groups)
            assert keys_got == want_keys, (packed, layout, [(p, keys_got[p], want_keys[p]) for p in range(len(want_keys)) if keys_got[p] != want_keys[p]][:5])
            assert info == want_info, (info, want_info)
            pk = [packed] * len(segments) if isinstance(packed, bool) else packed
            at = 0
            for p, (fields, off, s) in enumerate(written):      # the records, expanded, and their strings back to back
                seg, i = want_keys[p]
                assert s == segments[seg][i] and off == at and fields == expanded(sources[(seg, i)], pk[seg], s), (p, seg, i, fields, s)
                at += len(s)
            if by == STRING and want_info["findings"]:
                assert all(a >= b for a, b in zip([want_info["findings"]] + left, left)) and left[-1] == 0, left
            first = first or (keys_got, info, left)
            assert (keys_got, info, left) == first      # the rounds do not depend on the records' type, the layout or the grid
    if want_rounds is not None:
        assert want_info["rounds"] == want_rounds, want_info
    return want_keys, want_info


# ---- inputs

def boundary_strings():
    """every length 0..40; pairs that first differ at byte 7, 8, 9, 15, 16, 17; a string and its prefix at lengths 8 and 16;
    "a", "a\\0", "a\\0\\0"; 0x7F / 0x80 / 0xFF at a word's first and last byte"""
    rng = random.Random(40)
    out = [text(rng, n, b"abcXYZ\x00\x7f\x80\xff") for n in range(41)]
    stem = b"0123456789abcdefghijklmnop"
    for at in (7, 8, 9, 15, 16, 17):
        out += [stem[:at] + b"x" + stem[at + 1:], stem[:at] + b"y" + stem[at + 1:]]
    out += [stem[:8], stem[:8] + b"z", stem[:16], stem[:16] + b"z", stem[:8], stem[:16]]
    out += [b"a", b"a\x00", b"a\x00\x00", b"a\x00", b"a", b"a"]
    for b in (0x7F, 0x80, 0xFF):
        out += [bytes([b]) + b"1234567", b"1234567" + bytes([b]), b"12345678" + bytes([b]) + b"z", b"123456781234567" + bytes([b])]
    return out


def test_the_inputs_hold_what_they_are_meant_to():
    strings = boundary_strings()
    assert {len(s) for s in strings} >= set(range(41))
    ks = sorted(strings)
    first_difference = {lcp(a, b) for a in strings for b in strings if a != b and len(a) == len(b) and lcp(a, b) < len(a)}
    assert first_difference >= {7, 8, 9, 15, 16, 17}
    assert any(len(a) == 8 and b.startswith(a) and len(b) > 8 for a in strings for b in strings) and any(len(a) == 16 and b.startswith(a) and len(b) > 16 for a in strings for b in strings)
    assert ks.index(b"a") < ks.index(b"a\x00") < ks.index(b"a\x00\x00")
    _, info = model(strings, False, 0, True)
    assert info["rounds"] >= 3 and info["tied"] >= 6 and info["tied"] < len(strings)      # ties that need depth >= 2, classes and singletons
    assert max(strings.count(s) for s in strings) >= 3 and min(strings.count(s) for s in strings) == 1
    # bytes >= 0x80 sort behind ASCII, whatever a signed compare would say
    assert ks.index(b"1234567\x7f") < ks.index(b"1234567\x80") < ks.index(b"1234567\xff")


def test_word_and_rem_at_every_alignment_and_the_fold(core):
    """the word of the key: big-endian, zero-padded, rem = min(len - 8d, 8); at every address mod 8 (the loads), with the fold"""
    rng = random.Random(41)
    seen_alignments = set()
    for n in range(0, 42):
        s = bytes(rng.choice(b"@AZ[`az{\x00\x7f\x80\xc1\xda\xff") for _ in range(n))
        region, region_bytes = C.c_void_p(), C.c_uint64()
        base = core.sxs_guarded(max(n, 1), C.byref(region), C.byref(region_bytes))      # the string ends where the page without access begins
        try:
            at = base + (max(n, 1) - n)
            C.memmove(at, s, n)
            seen_alignments.add((at % 8, n >= 8))      # (the page's end is aligned: the string's first byte lies at -n mod 8)
            for depth in range(6):
                for nocase in (0, 1):
                    for desc in (0, 1):
                        w, rem = C.c_uint64(), C.c_uint32()
                        core.sxs_order_word(at, n, depth, nocase, desc, C.byref(w), C.byref(rem))
                        part = (fold(s) if nocase else s)[8 * depth:8 * depth + 8]
                        want_w, want_rem = int.from_bytes(part.ljust(8, b"\x00"), "big"), len(part)
                        if desc:
                            want_w, want_rem = want_w ^ (1 << 64) - 1, 8 - want_rem
                        assert (w.value, rem.value) == (want_w, want_rem), (n, depth, nocase, desc, s)
        finally:
            core.sxs_unmap(region, region_bytes)
    assert seen_alignments >= {(a, True) for a in range(8)}      # a full word at every address mod 8: the 8-byte, the 4-byte and the byte loads


def test_lengths_boundaries_prefixes_nuls_and_high_bytes(core):
    strings = boundary_strings()
    random.Random(42).shuffle(strings)
    for flags in (0, DESC):
        check(core, [strings], flags=flags)
    check(core, [strings[:50], strings[50:]], flags=0)


def test_classes_of_equal_strings_across_two_segments_keep_print_order(core):
    rng = random.Random(43)
    a = [text(rng, rng.randrange(0, 30), b"abc") for _ in range(150)]
    b = [text(rng, rng.randrange(0, 30), b"abc") for _ in range(90)]
    for k in (3, 70, 149):
        a[k] = b"in both segments, three and two times"
    b[5] = b[80] = b"in both segments, three and two times"
    want, info = check(core, [a, b])
    at = [p for p, (s, i) in enumerate(want) if (a, b)[s][i] == a[3]]
    assert [want[p] for p in at] == [(0, 3), (0, 70), (0, 149), (1, 5), (1, 80)] and at == list(range(at[0], at[0] + 5))
    want_desc, _ = check(core, [a, b], flags=DESC)
    at = [p for p, (s, i) in enumerate(want_desc) if (a, b)[s][i] == a[3]]
    assert [want_desc[p] for p in at] == [(0, 3), (0, 70), (0, 149), (1, 5), (1, 80)]      # descending leaves the ties in print order
    assert info["tied"] >= 5


def test_letter_case_under_the_fold(core):
    rng = random.Random(44)
    base = [text(rng, rng.randrange(3, 20), b"abcdXYZ9_") for _ in range(80)]
    strings = []
    for s in base:
        strings += [s, s.swapcase(), s.upper()][:rng.randrange(1, 4)]
    strings += [b"Ab", b"aB", b"AB", b"ab", b"k\xc0z", b"K\xe0Z", b"k@z", b"k`z", b"k[z", b"k{z"]
    plain, _ = check(core, [strings])
    folded, info = check(core, [strings], flags=NOCASE)
    assert plain != folded and info["tied"] >= 4
    at = [strings.index(s) for s in (b"Ab", b"aB", b"AB", b"ab")]
    where = [p for p, (_, i) in enumerate(folded) if i in at]
    assert [folded[p][1] for p in where] == at and where == list(range(where[0], where[0] + 4))      # one class, in print order
    check(core, [strings[:100], strings[100:]], flags=NOCASE | DESC)


def test_a_filter_that_drops_a_wavefronts_first_and_last_lane(core):
    rng = random.Random(45)
    strings = [text(rng, rng.randrange(0, 25), b"abcd") for _ in range(200)]
    labels = [[1 if i % 64 not in (0, 63) else 2 for i in range(200)]]
    want, info = check(core, [strings], labels, any_=1)
    assert info["findings"] == 200 - 7 and all(i % 64 not in (0, 63) for _, i in want)
    check(core, [strings], labels, none=1)                                # only the first and last lanes
    check(core, [strings], labels, any_=3, all_=2, flags=DESC)
    check(core, [strings], labels, any_=4, every=False)                    # nothing takes part
    two = [strings[:130], strings[130:]]
    check(core, two, [labels[0][:130], labels[0][130:]], any_=1)


@pytest.mark.parametrize("by", [STRING, FIELD])
def test_limits_around_the_number_of_findings(core, by):
    rng = random.Random(46)
    strings = [text(rng, rng.randrange(0, 12), b"ab") for _ in range(130)]
    labels = [[rng.randrange(6) << 32 | rng.randrange(4) for _ in range(130)]]
    n = 130
    for limit in (0, 1, n - 1, n, n + 1):
        _, info = check(core, [strings], labels, by=by, shift=32 if by == FIELD else 0, bits=32 if by == FIELD else 64, limit=limit, every=False)
        assert info["kept"] == (limit if 0 < limit < n else n) and info["findings"] == n


def test_the_label_field_as_a_number(core):
    rng = random.Random(47)
    strings = [text(rng, rng.randrange(1, 9), b"xyz") for _ in range(300)]
    labels = [[rng.choice((0, 1, 2, 3, 1 << 31, (1 << 32) - 1, rng.randrange(1 << 32))) << 32 | rng.randrange(1 << 32) for _ in range(300)]]
    for shift, bits in ((32, 32), (0, 32), (0, 64), (63, 1), (30, 5)):
        for flags in (0, DESC):
            _, info = check(core, [strings], labels, by=FIELD, flags=flags, shift=shift, bits=bits, every=False)
            assert info["rounds"] == 0 and info["max_depth"] == 0
    check(core, [strings[:100], strings[100:]], [labels[0][:100], labels[0][100:]], by=FIELD, shift=32, bits=32, flags=DESC, any_=1, limit=20)


def test_two_hundred_strings_that_share_four_thousand_bytes(core):
    rng = random.Random(48)
    stem = text(rng, 4000, b"abcdefgh")
    strings = [stem + text(rng, rng.randrange(0, 12), b"abAB") for _ in range(200)] + [b"short", stem[:100]]
    _, info = check(core, [strings], every=False)
    assert info["rounds"] >= 500 and info["max_depth"] == info["rounds"] - 1
    check(core, [strings[:90], strings[90:]], flags=NOCASE | DESC, every=False)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
def test_record_counts_around_a_wavefront(core, n):
    rng = random.Random(49 + n)
    strings = [text(rng, rng.randrange(0, 20), b"abc") for _ in range(n)]
    strings[-1] = strings[0]
    check(core, [strings])
    check(core, [strings], flags=DESC)


def test_nothing_at_all(core):
    keys, written, info, left, _ = run(core, [[b"x"]], labels=[[0]], any_=1)
    assert (keys, written, left) == ([], [], []) and info == dict(findings=0, kept=0, rounds=0, tied=0, max_depth=0)


def test_mission_ids_without_a_position0_are_not_needed_by_unpacked_segments(core):
    """an unpacked segment's records pass as they are: file id, slice index and mission id are the record's"""
    strings = [b"b", b"a", b"c", b"a"]
    keys, written, info, _, sources = run(core, [strings], packed=False)
    assert keys == [(0, 1), (0, 3), (0, 0), (0, 2)] and [w[2] for w in written] == [b"a", b"a", b"b", b"c"] and info["tied"] == 2
    assert [w[0][5] for w in written] == [3, 3, 3, 3]


# ---- the same lane functions under the address and undefined-behaviour sanitizers, as a program of their own

def test_a_sanitizer_build_orders_the_same():
    exe = built("order_core_main", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSXS_ORDER_MAIN"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "order core: ok", (out.stdout[-500:], out.stderr[-2000:])
