"""sx_result_select_device without a GPU: a host-only context has no device-resident result, so the selection is refused with
SX_E_STATE (the caller filters on the host); bad arguments are SX_E_INVALID, told apart from that."""
import ctypes as C
import random

import pytest

import refconfig as rc
import stringsext_amd as sx
from product_harness import oracle_runs_for_chunk
from test_host_logic import synth


def select_rc(sc, res, patterns, n=None, flags=0):
    arr = (sx.Pattern * max(1, len(patterns)))(*[sx.Pattern(p, ln) for p, ln in patterns])
    out = C.c_void_p(1)
    code = sx.lib().sx_result_select_device(sc.h, res.h, arr, len(patterns) if n is None else n, flags, C.byref(out))
    assert out.value is None          # *out = NULL on every error
    return code


def test_a_host_only_context_is_refused_and_bad_arguments_are_invalid():
    rng = random.Random(2026)
    data = synth(rng, 300_000, 1 / 300)
    ms = rc.missions(encodings=["utf-8", "utf-16le"], chars_min="10")
    sc = sx.Scanner(ms, device=sx.SX_HOST_ONLY, result_on_device=True)
    try:
        res = sc.replay_runs(data, oracle_runs_for_chunk(ms, data, 0), file_id=1)
        assert len(res) > 10
        for kw in (dict(), dict(ignore_case=True), dict(invert=True)):
            with pytest.raises(sx.SxError) as e:
                res.select_device(b"abc", **kw)
            assert e.value.code == sx.SX_E_STATE
        with pytest.raises(sx.SxError) as e:
            res.select_device([b"a", b"bc"])
        assert e.value.code == sx.SX_E_STATE
        # bad arguments are told apart from a result that is in the wrong place
        for bad in ([], [b"x"] * 17, [b""], [b"ok", b""], [b"y" * 65], b""):
            with pytest.raises(sx.SxError) as e:
                res.select_device(bad)
            assert e.value.code == sx.SX_E_INVALID, bad
        assert sx.SX_SELECT_MAX_PATTERNS == 16 and sx.SX_SELECT_MAX_PATTERN_BYTES == 64
        assert select_rc(sc, res, [(b"abc", 3)]) == sx.SX_E_STATE
        assert select_rc(sc, res, [(b"abc", 3)], flags=4) == sx.SX_E_INVALID              # an unknown flag bit
        assert select_rc(sc, res, [(b"abc", 3)], flags=3 | 1 << 31) == sx.SX_E_INVALID
        assert select_rc(sc, res, [(b"abc", 3)], n=0) == sx.SX_E_INVALID
        assert select_rc(sc, res, [(b"abc", 3)], n=-1) == sx.SX_E_INVALID
        assert select_rc(sc, res, [(None, 3)]) == sx.SX_E_INVALID                         # a NULL pattern
        out = C.c_void_p(1)
        assert sx.lib().sx_result_select_device(sc.h, res.h, None, 1, 0, C.byref(out)) == sx.SX_E_INVALID and out.value is None
        arr = (sx.Pattern * 1)(sx.Pattern(b"abc", 3))
        assert sx.lib().sx_result_select_device(sc.h, res.h, arr, 1, 0, None) == sx.SX_E_INVALID
        assert sx.lib().sx_result_select_device(sc.h, None, arr, 1, 0, C.byref(out)) == sx.SX_E_INVALID and out.value is None
        # the result is as good as before
        assert len(res.findings()) == len(res)
        res.free()
    finally:
        sc.close()
    with pytest.raises(sx.SxError) as e:      # a closed Scanner
        sx.Result(sc, None).select_device(b"abc")
    assert e.value.code == sx.SX_E_STATE
