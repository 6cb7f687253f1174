"""sx_result_fold_device, sx_labels_rebind (Result.fold_device, Labels.rebind): the strings of a result that lies in HBM folded by
Unicode simple case folding on the device, and what the other operations make of the fold — over the lines of tests/fold_plant.py.

The sources
    wave k     one UTF-8 Mission on the wave path, packed records, ONE segment of k findings: k = 1, 63, 64, 65, 129 — around a
               wavefront's 64 records and past two — and R + 1, R = CUs x kRowsGroupsPerCu x kRowsWaves x 64 read from the sources as
               tests/test_gpu_result_strides.py reads them: the one record of the kernels' second trip
    lane k     the same Mission on the lane-per-region replay, the lines behind the buffer's first window: unpacked records,
               strings where the writer put them; the small k
    merged     two Missions, `-e ascii -e utf-8`, under SX_MERGE_PART_FINDINGS=1024: packed, several segments, strings back to back

Every expected value is the oracle's text (result_plant.expected()) and fold_plant.fold() — the rule in Python — over its strings; no
value comes from a product Scanner."""
import ctypes as C
import re

import numpy as np
import pytest

import fold_plant as fp
import result_plant as rp
import stringsext_amd as sx
from test_gpu_result_strides import SeenModel, check_records, picked, printed_on_device, same, trip_sizes, words_of
from test_gpu_select_device import info_tuple

pytestmark = pytest.mark.gpu

FIRST, REPEATED, SEEN, SHIFT = sx.SX_DISTINCT_FIRST, sx.SX_DISTINCT_REPEATED, sx.SX_DISTINCT_SEEN, sx.SX_DISTINCT_COUNT_SHIFT
QUIET, TWO_WINDOWS = b"\x80", 2 * 4096      # a byte in which the Mission reads no character; the wave path takes buffers of two windows or more
SMALL = (1, 63, 64, 65, 129)
MERGED_LINES = 3000


class Src:
    def __init__(self, name, sc, res, rows):
        self.name, self.sc, self.res, self.rows = name, sc, res, rows
        self.folded = [fp.fold(s) for s in rows.strs]
        self.frows = rows.take(np.arange(rows.n), strs=self.folded)

    def folded_text(self):
        """the oracle's text with every string folded"""
        raw = [r[:len(r) - len(s)] + f for r, s, f in zip(self.rows.raw, self.rows.strs, self.folded)]
        return rp.OUTPUT_BOM + b"".join(b"\n" + r for r in raw) + b"\n"

    def close(self):
        self.res.free(); self.sc.close()


def make(kind, k):
    env, kw = (), {}
    if kind == "merged":
        ms, data, env = fp.ms2(), fp.buffer(k), (("SX_MERGE_PART_FINDINGS", "1024"), ("SX_MERGE_PART_MIB", "1"))
    else:
        ms, data = fp.ms1(), fp.buffer(k)
        if kind == "lane":      # (the buffer's first window is replayed by the host: the lines lie behind it, where the device writes them)
            data = QUIET * 4096 + data
        data += QUIET * max(0, TWO_WINDOWS - len(data))
        env, kw = ((("SX_WAVE_REPLAY", "1"),), {}) if kind == "wave" else ((("SX_WAVE_REPLAY", "0"),), dict(device_replay=True))
    rows = rp.expected(ms, data)
    with pytest.MonkeyPatch.context() as mp:
        for key, v in env:
            mp.setenv(key, v)
        sc = sx.Scanner(ms, device=0, result_on_device=True, **kw)      # (a context keeps the switches it was created under)
    res = sc.scan(data, file_id=1)
    segs = res.device_segments()
    assert len(res) == rows.n and all(g[0] for g in segs), (kind, k, len(res), rows.n)
    assert [g[4] for g in segs] == [kind != "lane"] * len(segs), (kind, [g[4] for g in segs])
    if kind == "merged":
        assert len(segs) >= 3 and rows.n > k
    else:
        assert rows.n == k and (kind == "lane" or len(segs) == 1), (kind, k, rows.n, len(segs))
    return Src("%s %d" % (kind, k), sc, res, rows)


@pytest.fixture(scope="module")
def sources():
    made = {}

    def get(kind, k):
        if (kind, k) not in made:
            made[kind, k] = make(kind, k)
        return made[kind, k]
    yield get
    for s in made.values():
        s.close()


def raw_records(sc, res):
    """per segment (packed, the records as rows of bytes)"""
    out = []
    for fp_, n, ap, alen, packed, info in res.device_segments():
        size = 16 if packed else 32
        out.append((packed, np.frombuffer(sc.download(fp_, n * size), dtype=np.uint8).reshape(n, size)))
    return out


def check_fold(s, res, fold, rows=None, frows=None):
    """(a) and (c): `fold`, folded from `res` whose rows are `rows`: segment for segment the source's shape, record for record the
    source's fields, the strings fold_plant.fold() of the oracle's, back to back; the info"""
    rows, frows = rows or s.rows, frows or s.frows
    src, got = res.device_segments(), fold.device_segments()
    assert [(g[1], g[4], info_tuple(g[5])) for g in got] == [(g[1], g[4], info_tuple(g[5])) for g in src], s.name
    for g in got:
        assert g[0] % 256 == 0 and g[2] == g[0] + g[1] * (16 if g[4] else 32)                      # [records][strings], 256-byte aligned
    check_records(s.sc, fold, frows, True, s.name + ": fold")
    for (packed, a), (_, b) in zip(raw_records(s.sc, res), raw_records(s.sc, fold)):
        keep = np.ones(a.shape[1], dtype=bool)
        keep[8:14 if packed else 16] = False                                                        # str_off and str_len
        assert np.array_equal(a[:, keep], b[:, keep]), s.name                                       # every other byte of every record
    want = dict(findings=rows.n, bytes_in=sum(len(x) for x in rows.strs), bytes_out=sum(len(x) for x in frows.strs),
                changed=sum(1 for x, y in zip(rows.strs, frows.strs) if x != y))
    assert fold.fold_info == want, (s.name, fold.fold_info, want)
    return want


def check_printed(s, fold):
    got, want = printed_on_device(s.sc, fold), s.folded_text()
    assert len(got) == len(want) and got == want, (s.name, len(got), len(want))


@pytest.mark.parametrize("k", SMALL)
@pytest.mark.parametrize("kind", ["wave", "lane"])
def test_the_fold_of_one_mission_around_a_wavefront(sources, kind, k):
    s = sources(kind, k)
    fold = s.res.fold_device()
    info = check_fold(s, s.res, fold)
    assert k < 63 or (0 < info["changed"] < k and info["bytes_in"] != info["bytes_out"])
    check_printed(s, fold)
    # the fold is idempotent: the fold of the fold has its strings, and changes none
    again = fold.fold_device()
    check_records(s.sc, again, s.frows, True, s.name + ": fold of the fold")
    assert again.fold_info == dict(findings=k, bytes_in=info["bytes_out"], bytes_out=info["bytes_out"], changed=0)
    again.free(); fold.free()


def test_the_fold_of_merged_missions_in_several_segments(sources):
    s = sources("merged", MERGED_LINES)
    fold = s.res.fold_device()
    check_fold(s, s.res, fold)
    check_printed(s, fold)
    fold.free()


def test_one_record_in_the_second_trip(sources):
    r, _ = trip_sizes()
    s = sources("wave", r + 1)
    fold = s.res.fold_device()
    info = check_fold(s, s.res, fold)
    assert info["findings"] == r + 1 and 0 < info["changed"] < r
    check_printed(s, fold)
    fold.free()


@pytest.fixture(scope="module")
def merged(sources):
    return sources("merged", MERGED_LINES)


@pytest.fixture(scope="module")
def lane(sources):
    return sources("lane", 129)


def test_distinct_on_the_fold_joins_what_the_ascii_fold_keeps_apart(merged):
    s = merged
    want, want_info, keys, _ = rp.distinct_model(s.folded, FIRST, REPEATED, SHIFT)
    ascii_words, ascii_info, _, _ = rp.distinct_model(s.rows.strs, FIRST, REPEATED, SHIFT, nocase=True)
    assert want_info["distinct"] < ascii_info["distinct"] - 100
    fold = s.res.fold_device()
    lab = fold.distinct_device()
    got = words_of(s.sc, lab, fold)
    same(got, want, s.name + ": distinct words of the fold", s.folded)
    assert {k: lab.info[k] for k in ("findings", "distinct", "repeated")} == want_info
    plain = s.res.distinct_device(ignore_case=True)
    same(words_of(s.sc, plain, s.res), ascii_words, s.name + ": distinct words under the ASCII fold", s.rows.strs)
    assert not np.array_equal(got, ascii_words)
    # sort -u whatever the case: the first finding of every class, as it was written — the labels of the fold, bound to the source
    first = want & np.uint64(FIRST) != 0
    bound = lab.rebind(s.res)
    sel = s.res.select_device(bound, any=FIRST)
    kept = s.rows.take(first)
    check_records(s.sc, sel, kept, True, s.name + ": the classes' first findings")
    assert [fp.fold(x) for x in kept.strs] == keys
    # ... and the five largest classes, by the count in the rebound words
    top = s.res.order_device("field", labels=bound, shift=SHIFT, bits=32, descending=True, any=FIRST, limit=5)
    sizes = (want >> np.uint64(SHIFT)).astype(np.int64)
    order = sorted(np.nonzero(first)[0].tolist(), key=lambda i: -int(sizes[i]))[:5]
    assert [(f["position"], f["s"].encode()) for f in top.findings()] == [(int(s.rows.position[i]), s.rows.strs[i]) for i in order]
    top.free(); sel.free(); bound.free(); plain.free(); lab.free(); fold.free()


@pytest.mark.parametrize("which", ["merged", "lane"])
def test_grep_i_in_every_script(which, request):
    s = request.getfixturevalue(which)
    needles = [fp.fold(n.encode()) for n in fp.NEEDLES]
    assert needles[0] == sx.fold("ПАРОЛЬ".encode()) == "пароль".encode()
    words = np.array([sum(1 << p for p, n in enumerate(needles) if n in f) for f in s.folded], dtype=np.uint64)
    ls = s.sc.label_set([sx.fold(n.encode()) for n in fp.NEEDLES])
    fold = s.res.fold_device()
    lab = fold.label_device(ls)
    same(words_of(s.sc, lab, fold), words, s.name + ": labels of the fold", s.folded)
    bound = lab.rebind(s.res)
    assert [n for _, n in bound.device_segments()] == [g[1] for g in s.res.device_segments()]
    same(words_of(s.sc, bound, s.res), words, s.name + ": the rebound labels", s.rows.strs)
    # the new labels are the source's and no longer the fold's, the old ones the other way round
    for res, labels in ((fold, bound), (s.res, lab)):
        with pytest.raises(sx.SxError) as e:
            res.select_device(labels, any=1)
        assert e.value.code == sx.SX_E_INVALID
    for masks in (dict(any=1), dict(any=0b0110), dict(all=0b1001), dict(any=1, none=0b1000)):
        mask = picked(words, masks.get("any", 0), masks.get("all", 0), masks.get("none", 0))
        sel = s.res.select_device(bound, **masks)
        want = s.rows.take(mask)
        assert len(sel) == want.n
        if want.n:
            check_records(s.sc, sel, want, True, "%s: grep -i %r" % (s.name, masks))            # the ORIGINAL strings
        sel.free()
    # the plain selection finds fewer: the needle stands in the source in several spellings
    hit = picked(words, 1, 0, 0)
    exact = s.rows.mask(lambda x: fp.NEEDLES[0].encode() in x)
    nocase = s.rows.mask(lambda x: fp.NEEDLES[0].encode().lower() in x.lower())
    assert which == "lane" or exact.sum() == nocase.sum() < hit.sum()
    # the range selection takes the rebound labels too
    sel = s.res.select_range_device(bound, 0, 4, 1, 1)
    assert len(sel) == int((words == 1).sum())
    sel.free()
    bound.free(); lab.free(); fold.free(); ls.free()


def test_order_and_seen_on_the_fold(merged):
    s = merged
    fold = s.res.fold_device()
    # LC_ALL=C sort of the folded strings; ties keep print order
    order = sorted(range(s.rows.n), key=lambda i: s.folded[i])
    out = fold.order_device(limit=2000)
    got = out.findings()
    assert [(f["position"], f["s"].encode()) for f in got] == [(int(s.rows.position[i]), s.folded[i]) for i in order[:2000]]
    assert out.order_info["findings"] == s.rows.n and out.order_info["kept"] == 2000
    out.free()
    # the seen set remembers folded strings
    model, distinct = SeenModel(), rp.distinct_model(s.folded, FIRST, REPEATED, SHIFT)
    full = SeenModel()
    full.expect(distinct)
    cap = full.held_info()
    ss = s.sc.seen_set(cap["strings"], cap["bytes"])
    for call in range(2):
        want, want_info = model.expect(distinct)
        lab = fold.seen_device(ss)
        same(words_of(s.sc, lab, fold), want, "%s: seen words of the fold, call %d" % (s.name, call), s.folded)
        assert {k: lab.info[k] for k in want_info} == want_info
        assert bool((want & np.uint64(SEEN)).all()) == (call == 1)
        lab.free()
    # a string in another spelling is held already: the source's own strings, folded on the host
    info = ss.info()
    assert (info["strings"], info["bytes"]) == (cap["strings"], cap["bytes"])
    assert all(ss.contains([sx.fold(x) for x in s.rows.strs[:50]]))
    ss.free(); fold.free()


def test_the_fold_of_a_selection_and_of_an_extraction(merged):
    s = merged
    needle = "П".encode()
    mask = s.rows.mask(lambda x: needle in x)
    assert 0 < mask.sum() < s.rows.n
    sel = s.res.select_device(needle)
    fold = sel.fold_device()
    rows = s.rows.take(mask)
    frows = rows.take(np.arange(rows.n), strs=[fp.fold(x) for x in rows.strs])
    check_fold(s, sel, fold, rows, frows)
    fold.free(); sel.free()
    # grep -o, then the fold: the matches, folded
    pattern = rb"[A-Za-z]{3,}"
    rx = re.compile(pattern)
    per_class = [rx.findall(u) for u in s.rows.uniq]
    count = np.array([len(m) for m in per_class], dtype=np.int64)[s.rows.inv]
    matches = [m for u in s.rows.inv.tolist() for m in per_class[u]]
    assert any(m != m.lower() for m in matches)
    rows = s.rows.take(np.repeat(np.arange(s.rows.n), count), strs=matches)
    frows = rows.take(np.arange(rows.n), strs=[fp.fold(x) for x in matches])
    xs = s.sc.extract_set([pattern])
    ext = s.res.extract_device(xs)
    fold = ext.fold_device()
    check_fold(s, ext, fold, rows, frows)
    fold.free(); ext.free(); xs.free()


def test_refusals_are_decided_before_anything_is_launched(merged, lane):
    s, L = merged, sx.lib()
    out, info = C.c_void_p(0xDEAD0), sx.FoldInfo()
    # a flag
    assert L.sx_result_fold_device(s.sc.h, s.res.h, 1, C.byref(out), C.byref(info)) == sx.SX_E_INVALID and out.value is None
    assert b"SX_FOLD_SIMPLE" in L.sx_last_error(s.sc.h)
    # rebind onto a result of another shape: other record counts, other segment counts
    fold = s.res.fold_device()
    lab = fold.distinct_device()
    sel = s.res.select_device(b"a")
    assert 0 < len(sel) < len(s.res)
    with pytest.raises(sx.SxError) as e:
        lab.rebind(sel)
    assert e.value.code == sx.SX_E_INVALID
    with pytest.raises(sx.SxError) as e:
        lab.rebind(lane.res)                   # (another context's result is none of this context's blocks)
    assert e.value.code == sx.SX_E_STATE
    # the blocks take turns: `fold` lies in the block that the next selection writes — it was made two calls ago
    out = C.c_void_p(0xDEAD0)
    assert L.sx_result_fold_device(s.sc.h, fold.h, 0, C.byref(out), None) == sx.SX_E_STATE and out.value is None
    assert b"two calls ago" in L.sx_last_error(s.sc.h)
    lab.rebind(fold).free()                    # (still valid: the refused call aged nothing, and a rebind ages nothing)
    s.res.select_device(b"a").free()           # now `fold` is gone ...
    with pytest.raises(sx.SxError) as e:
        lab.rebind(fold)                       # ... and nothing binds to it
    assert e.value.code == sx.SX_E_STATE
    sel.free(); lab.free(); fold.free()
    # as many findings in ONE segment: the order's output
    ordered = s.res.order_device()
    fold = s.res.fold_device()
    lab = fold.distinct_device()
    assert len(ordered) == len(fold) and len(ordered.device_segments()) == 1 < len(fold.device_segments())
    with pytest.raises(sx.SxError) as e:
        lab.rebind(ordered)
    assert e.value.code == sx.SX_E_INVALID
    lab.free(); fold.free(); ordered.free()
    # a result in host memory
    host = sx.Scanner(fp.ms1(), device=0)
    try:
        res = host.scan(fp.buffer(65), file_id=1)
        assert len(res) == 65
        out = C.c_void_p(0xDEAD0)
        assert L.sx_result_fold_device(host.h, res.h, 0, C.byref(out), None) == sx.SX_E_STATE and out.value is None
        assert b"host memory" in L.sx_last_error(host.h)
        with pytest.raises(sx.SxError) as e:
            res.fold_device()
        assert e.value.code == sx.SX_E_STATE
        res.free()
    finally:
        host.close()
