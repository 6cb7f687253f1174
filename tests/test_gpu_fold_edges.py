"""sx_result_fold_device where only the device can go wrong, over the lines tests/fold_plant.py plants for it (tests/test_fold_plant.py
asserts on the CPU what they hold):

    pages      fold_plant.page_lines(): every code point of every page of the table that fold_load copies into LDS — the last three
               pages in its loop's second trip —, the code points next to a page that lie on none (kFoldNoPage), and code points at and
               above kFoldLimit, which must not look into the index at all
    cuts       fold_plant.split_lines() extracted with SPLIT_PATTERNS: matches that end in a lead byte, or in a lead byte and some of
               its continuation bytes, in front of matches that begin with the others — back to back in the arena, so that only
               `left < n` in fold_decode keeps a lane from folding a character that two records share
    long       fold_plant.long_lines(255) on the lane-per-region replay, long_lines(1024) merged and packed, limit_lines() at `-q 16000`:
               folded str_len of 48 000 and 64 000 in packed records, wave_prefix over lengths of tens of thousands, and 8-byte words
               of ASCII that go out by each of FoldWrite::word's three stores
    counts     the record counts of tests/test_gpu_result_edges.py that tests/test_gpu_fold_device.py lacks, R — the measure kernel's
               extra wavefront alone in trip 2 — and R + 513: two trips that both add to a wavefront's totals before its one atomic
    order      the fold of an order's output (one segment, strings as order_part_strings laid them) and the order of the fold

and for every source the host twin sx_fold_utf8 (stringsext_amd.fold, with which a caller folds its patterns) against the device's
strings, all of them, as one comparison of the joined bytes.

Every expected value is the oracle's text (result_plant.expected()) with fold_plant.fold() — the rule in Python — over its strings; no
value comes from a product Scanner."""
import numpy as np
import pytest

import fold_plant as fp
import long_plant as lp
import result_plant as rp
import stringsext_amd as sx
from test_gpu_fold_device import QUIET, TWO_WINDOWS, Src, check_fold, check_printed, make, raw_records
from test_gpu_result_edges import EDGES
from test_gpu_result_on_device_multi import F16, F32
from test_gpu_result_strides import check_records, same, trip_sizes, words_of

pytestmark = pytest.mark.gpu

FIRST, REPEATED, SHIFT = sx.SX_DISTINCT_FIRST, sx.SX_DISTINCT_REPEATED, sx.SX_DISTINCT_COUNT_SHIFT
PARTS = (("SX_MERGE_PART_FINDINGS", "1024"), ("SX_MERGE_PART_MIB", "1"))
COUNTS = [k for k in EDGES if k not in (1, 63, 64, 65, 129)]
# (everything of a buffer of two lines lies in the host's entry part: no lane source, tests/test_gpu_result_edges.py)
COUNT_SPECS = [("wave", k) for k in COUNTS] + [("lane", k) for k in COUNTS if k > 2]


def make_from(name, kind, ms, data, env=()):
    """test_gpu_fold_device.make() for any Missions and lines.  kind: `wave` (packed, one segment), `lane` (the lane-per-region replay:
    unpacked, the lines behind the buffer's first window) or `merged` (several Missions: packed, strings back to back)"""
    kw = {}
    if kind == "lane":
        data, env, kw = QUIET * 4096 + data, (("SX_WAVE_REPLAY", "0"),), dict(device_replay=True)
    elif kind == "wave":
        env = (("SX_WAVE_REPLAY", "1"),)
    if kind != "merged":
        data += QUIET * max(0, TWO_WINDOWS - len(data))
    rows = rp.expected(ms, data)
    with pytest.MonkeyPatch.context() as mp:
        for key, v in env:
            mp.setenv(key, v)
        sc = sx.Scanner(ms, device=0, result_on_device=True, **kw)      # (a context keeps the switches it was created under)
    res = sc.scan(data, file_id=1)
    segs = res.device_segments()
    assert len(res) == rows.n and all(g[0] for g in segs), (name, len(res), rows.n)
    assert [g[4] for g in segs] == [kind != "lane"] * len(segs), (name, [g[4] for g in segs])
    assert (len(ms) > 1) == (kind == "merged") and (kind != "wave" or len(segs) == 1)
    return Src(name, sc, res, rows)


MAKERS = {
    "pages wave": lambda: make_from("pages wave", "wave", fp.ms1(), lp.buffer(fp.page_lines())),
    "pages lane": lambda: make_from("pages lane", "lane", fp.ms1(), lp.buffer(fp.page_lines())),
    "cuts merged": lambda: make_from("cuts merged", "merged", fp.ms2v(), fp.split_buffer(), PARTS),
    "cuts lane": lambda: make_from("cuts lane", "lane", fp.ms1(), lp.buffer(fp.split_lines())),
    "long 255": lambda: make_from("long 255", "lane", lp.msl1(), lp.buffer(fp.long_lines(255))),
    "long 1024": lambda: make_from("long 1024", "merged", fp.msl(), lp.buffer(fp.long_lines(1024))),
    "limit": lambda: make_from("limit", "merged", lp.limit_ms(), lp.buffer(fp.limit_lines())),
    "merged": lambda: make("merged", fp.SPLIT_BEHIND),
}


@pytest.fixture(scope="module")
def sources():
    made = {}

    def get(name):
        if name not in made:
            made[name] = MAKERS[name]()
        return made[name]
    yield get
    for s in made.values():
        s.close()


def arena_bytes(sc, res):
    return b"".join(sc.download(g[2], g[3]) for g in res.device_segments())


def fold_checked(s, res=None, rows=None, frows=None):
    """res.fold_device(), checked: check_fold — every record, every string, the info — and the host twin: sx_fold_utf8 over the oracle's
    strings is the fold's arenas, joined (its strings lie back to back in record order).  The twin folds the strings in one call, a
    \\n between them: no sequence of UTF-8 goes on across an ASCII byte, so that is every string folded on its own, ill-formed ends
    and beginnings included"""
    res, rows, frows = res or s.res, rows or s.rows, frows or s.frows
    fold = res.fold_device()
    info = check_fold(s, res, fold, rows, frows)
    together = b"\n".join(rows.strs)
    assert together.count(b"\n") == rows.n - 1
    twin = sx.fold(together).replace(b"\n", b"")
    got = arena_bytes(s.sc, fold)
    assert len(got) == len(twin) == info["bytes_out"] and got == twin, (s.name, len(got), len(twin))
    return fold, info


def folded_rows(rows, index=None):
    """`rows` (those `index` names), their strings folded"""
    rows = rows if index is None else rows.take(np.asarray(index, dtype=np.int64))
    return rows.take(np.arange(rows.n), strs=[fp.fold(x) for x in rows.strs])


def in_order(frows):
    """LC_ALL=C sort of folded rows; ties keep their order"""
    order = sorted(range(frows.n), key=lambda i: frows.strs[i])
    return frows.take(np.array(order, dtype=np.int64), strs=[frows.strs[i] for i in order])


# ---- 1. every page of the table, and what lies next to it

@pytest.mark.parametrize("kind", ["wave", "lane"])
def test_every_page_of_the_table_and_its_neighbours(sources, kind):
    s = sources("pages " + kind)
    assert s.rows.strs == fp.page_lines()
    fold, info = fold_checked(s)
    changed = sum(fp.fold(x) != x for x in fp.page_lines())
    assert info["changed"] == changed > 60 and info["findings"] == 96
    check_printed(s, fold)
    again = fold.fold_device()
    check_records(s.sc, again, s.frows, True, s.name + ": fold of the fold")
    assert again.fold_info == dict(findings=96, bytes_in=info["bytes_out"], bytes_out=info["bytes_out"], changed=0)
    again.free(); fold.free()


# ---- 2. characters cut in two by an extraction

def extracted(s):
    """(the extraction of SPLIT_PATTERNS from s.res, its rows by Python's re over the oracle's strings)"""
    rx = fp.split_rx()
    per_class = [rx.findall(u) for u in s.rows.uniq]
    count = np.array([len(m) for m in per_class], dtype=np.int64)[s.rows.inv]
    matches = [m for u in s.rows.inv.tolist() for m in per_class[u]]
    found, cuts = fp.split_pairs(s.rows.strs)
    assert found == matches and len(cuts) == 6 and min(cuts.values()) >= 2, cuts
    assert b"\xc8" in matches and b"\xba" in matches and matches[-1] == b"EN8\xd0"
    rows = s.rows.take(np.repeat(np.arange(s.rows.n), count), strs=matches)
    xs = s.sc.extract_set(fp.SPLIT_PATTERNS)
    ext = s.res.extract_device(xs)
    xs.free()
    check_records(s.sc, ext, rows, True, s.name + ": the matches")
    return ext, rows


def test_cut_sequences_back_to_back_in_several_segments(sources):
    s = sources("cuts merged")
    assert len(s.res.device_segments()) >= 3
    ext, rows = extracted(s)
    assert len(ext.device_segments()) >= 3 and rows.strs[-1][-1] == 0xD0           # the last segment's last match ends in a lead byte
    frows = folded_rows(rows)
    fold, info = fold_checked(s, ext, rows, frows)
    # (no match holds a whole character of two bytes or more: every one keeps its length, which a lane that read on would not)
    assert 0 < info["changed"] < rows.n and info["bytes_in"] == info["bytes_out"]
    # what the other operations make of these strings: sort | uniq -c, and LC_ALL=C sort
    want, want_info, _, _ = rp.distinct_model(frows.strs, FIRST, REPEATED, SHIFT)
    lab = fold.distinct_device()
    same(words_of(s.sc, lab, fold), want, s.name + ": distinct words of the folded matches", frows.strs)
    assert {k: lab.info[k] for k in ("findings", "distinct", "repeated")} == want_info
    lab.free()
    out = fold.order_device()
    check_records(s.sc, out, in_order(frows), True, s.name + ": the folded matches in order")
    out.free(); fold.free(); ext.free()


def test_cut_sequences_from_unpacked_records(sources):
    s = sources("cuts lane")
    assert s.rows.strs == fp.split_lines()
    ext, rows = extracted(s)
    fold, info = fold_checked(s, ext, rows, folded_rows(rows))
    assert 0 < info["changed"] < rows.n and info["bytes_in"] == info["bytes_out"]
    fold.free(); ext.free()


# ---- 3. long strings

def word_stores(s, res, fold, strs):
    """fold_plant.word_stores() of `res`'s strings and their places in `fold`: from the records' str_off, which check_fold has seen,
    and the arenas' addresses"""
    src, dst = [], []
    for (packed, a), (_, b), gs, gf in zip(raw_records(s.sc, res), raw_records(s.sc, fold), res.device_segments(), fold.device_segments()):
        kind = F16 if packed else F32
        src.append(gs[2] + a.view(kind)["str_off"].reshape(-1).astype(np.int64))
        dst.append(gf[2] + b.view(kind)["str_off"].reshape(-1).astype(np.int64))
    return fp.word_stores(strs, np.concatenate(src), np.concatenate(dst))


@pytest.mark.parametrize("name", ["long 255", "long 1024", "limit"])
def test_long_strings_that_grow_shrink_and_stay(sources, name):
    s = sources(name)
    lines = {"long 255": lambda: fp.long_lines(255), "long 1024": lambda: fp.long_lines(1024), "limit": fp.limit_lines}[name]()
    assert all(x in s.rows.strs for x in lines)
    fold, info = fold_checked(s)
    assert info["bytes_out"] < info["bytes_in"] and info["changed"] >= 8
    check_printed(s, fold)
    stores = word_stores(s, s.res, fold, s.rows.strs)
    print("%s: words of ASCII to an 8-aligned place, a 4-aligned one, neither: %r" % (name, stores))
    assert min(stores) > 0, (name, stores)
    if name == "limit":
        (packed, recs), = raw_records(s.sc, fold)
        lens = recs.view(F16)["str_len"].reshape(-1).tolist()
        assert packed and lens.count(48000) == 1 and lens.count(64000) == 1 and max(lens) == 64000
    fold.free()


def test_a_selection_whose_fold_is_longer(sources):
    s = sources("long 1024")
    needle = "\u023A".encode()
    mask = s.rows.mask(lambda x: needle in x)
    rows = s.rows.take(mask)
    sel = s.res.select_device(needle)
    fold, info = fold_checked(s, sel, rows, folded_rows(rows))
    assert info["findings"] == 9 + 8 and info["bytes_out"] > info["bytes_in"]
    fold.free(); sel.free()


def test_the_folded_limit_source_in_order_and_selected(sources):
    s = sources("limit")
    fold, _ = fold_checked(s)
    out = fold.order_device()
    check_records(s.sc, out, in_order(s.frows), True, "limit: the fold in order")
    out.free(); fold.free()
    fold = s.res.fold_device()                   # (the blocks take turns: the next call writes where the first fold lay)
    needle = sx.fold("\u023A\u023A\u023A\u023A".encode())
    assert needle == "\u2C65\u2C65\u2C65\u2C65".encode()
    mask = np.array([needle in f for f in s.folded], dtype=bool)
    assert mask.sum() == 1 and s.folded[int(np.argmax(mask))] == needle * 4000 and not s.rows.mask(lambda x: needle in x).any()
    sel = fold.select_device(needle)
    check_records(s.sc, sel, s.frows.take(np.nonzero(mask)[0], strs=[f for f, m in zip(s.folded, mask) if m]), True, "limit: the grown line, selected")
    assert len(sel.findings()) == 1 and int(s.frows.length[mask][0]) == 48000
    sel.free(); fold.free()


# ---- 4. record counts on a wavefront's and a workgroup's edge, and second trips

@pytest.mark.parametrize("kind,k", COUNT_SPECS, ids=["%s-%d" % spec for spec in COUNT_SPECS])
def test_the_fold_at_a_count_on_an_edge(kind, k):
    s = make(kind, k)
    try:
        fold, info = fold_checked(s)
        assert info["findings"] == k
        check_printed(s, fold)
        fold.free()
    finally:
        s.close()


@pytest.mark.parametrize("over", [0, 513])
def test_full_trips(over):
    """R records: the measure kernel's extra wavefront is alone in trip 2.  R + 513: trip 2 holds nine wavefronts of records, one of
    them partial, so the first wavefronts add a second trip's records to n_changed, bytes_in and the longest before their atomics"""
    r, _ = trip_sizes()
    s = make("wave", r + over)
    try:
        if over:
            late = [(x, f) for x, f in zip(s.rows.strs[r:], s.folded[r:])]
            assert len(late) == over and sum(x != f for x, f in late) > 64 and sum(len(x) - len(f) for x, f in late) != 0
        fold, info = fold_checked(s)
        assert info["findings"] == r + over and 0 < info["changed"] < r
        check_printed(s, fold)
        fold.free()
    finally:
        s.close()


# ---- 5. the fold of an order's output

def test_the_fold_of_an_order_and_the_order_of_the_fold(sources):
    """The order's output is one segment whose strings order_part_strings laid: its fold is, record for record, the fold of the
    source's records in that order.  Ordered again it has the strings of the source's fold, ordered, record for record; where two
    folded strings are equal the tie keeps the order of what was ordered, so the records' other fields are each order's own."""
    s = sources("merged")
    by_bytes = sorted(range(s.rows.n), key=lambda i: s.rows.strs[i])
    rows = s.rows.take(np.array(by_bytes, dtype=np.int64), strs=[s.rows.strs[i] for i in by_bytes])
    ordered = s.res.order_device()
    assert len(ordered.device_segments()) == 1 < len(s.res.device_segments())
    check_records(s.sc, ordered, rows, True, s.name + ": in order")
    frows = folded_rows(rows)
    assert frows.strs != sorted(frows.strs)                                       # the fold of an order is in no order
    fold, info = fold_checked(s, ordered, rows, frows)
    assert info["changed"] == sum(x != f for x, f in zip(s.rows.strs, s.folded))
    again = fold.order_device()
    check_records(s.sc, again, in_order(frows), True, s.name + ": the fold of the order, ordered")
    again.free(); fold.free(); ordered.free()
    fold, _ = fold_checked(s)
    out = fold.order_device()
    want = in_order(s.frows)
    check_records(s.sc, out, want, True, s.name + ": the fold, ordered")
    assert want.strs == in_order(frows).strs == sorted(s.folded)
    out.free(); fold.free()
