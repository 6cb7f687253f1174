"""sx_select_set_create and sx_result_select_set_device without a GPU: a host-only context has no device for a set's table and no
device-resident result, so both are refused with SX_E_STATE; bad arguments are SX_E_INVALID, told apart from that; and the list
selection's limits are where they were."""
import ctypes as C
import random

import pytest

import refconfig as rc
import stringsext_amd as sx
from product_harness import oracle_runs_for_chunk
from test_host_logic import synth


def create_rc(sc, patterns, n=None, flags=0):
    arr = (sx.Pattern * max(1, len(patterns)))(*[sx.Pattern(p, ln) for p, ln in patterns])
    out = C.c_void_p(1)
    code = sx.lib().sx_select_set_create(sc.h, arr, len(patterns) if n is None else n, flags, C.byref(out))
    assert code != sx.SX_OK and out.value is None          # *out = NULL on every error
    return code


def test_a_host_only_context_is_refused_and_bad_arguments_are_invalid():
    L = sx.lib()
    rng = random.Random(2027)
    data = synth(rng, 300_000, 1 / 300)
    ms = rc.missions(encodings=["utf-8", "utf-16le"], chars_min="10")
    sc = sx.Scanner(ms, device=sx.SX_HOST_ONLY, result_on_device=True)
    try:
        res = sc.replay_runs(data, oracle_runs_for_chunk(ms, data, 0), file_id=1)
        assert len(res) > 10
        # a set that could be built has no device to lie on
        for kw in (dict(), dict(ignore_case=True)):
            with pytest.raises(sx.SxError) as e:
                sc.pattern_set([b"abc", b"de"], **kw)
            assert e.value.code == sx.SX_E_STATE
        assert create_rc(sc, [(b"abc", 3)]) == sx.SX_E_STATE
        assert create_rc(sc, [(b"q" * 255, 255)] * 4112 + [(b"q" * 16, 16)]) == sx.SX_E_STATE      # 1 MiB in all
        # bad arguments are told apart from that
        for bad in ([], [b""], [b"ok", b""], [b"y" * 256], [b"q" * 255] * 4112 + [b"q" * 17]):
            with pytest.raises(sx.SxError) as e:
                sc.pattern_set(bad)
            assert e.value.code == sx.SX_E_INVALID, bad[:2]
        assert create_rc(sc, [(b"abc", 3)], n=0) == sx.SX_E_INVALID
        assert create_rc(sc, [(b"abc", 3)] * 2, n=65537) == sx.SX_E_INVALID                 # (refused before a pattern is read)
        assert create_rc(sc, [(b"abc", 3)], flags=sx.SX_SELECT_INVERT) == sx.SX_E_INVALID   # the set takes the fold, the call the inversion
        assert create_rc(sc, [(b"abc", 3)], flags=4) == sx.SX_E_INVALID
        assert create_rc(sc, [(b"abc", 3)], flags=1 | 1 << 31) == sx.SX_E_INVALID
        assert create_rc(sc, [(None, 3)]) == sx.SX_E_INVALID                                # a NULL pattern
        out = C.c_void_p(1)
        assert L.sx_select_set_create(sc.h, None, 1, 0, C.byref(out)) == sx.SX_E_INVALID and out.value is None
        arr = (sx.Pattern * 1)(sx.Pattern(b"abc", 3))
        assert L.sx_select_set_create(sc.h, arr, 1, 0, None) == sx.SX_E_INVALID
        assert L.sx_select_set_create(None, arr, 1, 0, C.byref(out)) == sx.SX_E_INVALID and out.value is None
        # the selection: NULL pointers (no set can exist here)
        out = C.c_void_p(1)
        assert L.sx_result_select_set_device(sc.h, res.h, None, 0, C.byref(out)) == sx.SX_E_INVALID and out.value is None
        out = C.c_void_p(1)
        assert L.sx_result_select_set_device(None, res.h, None, 0, C.byref(out)) == sx.SX_E_INVALID and out.value is None
        info = sx.SelectSetInfo()
        assert L.sx_select_set_info_get(None, C.byref(info)) == sx.SX_E_INVALID
        L.sx_select_set_free(None)                                                           # (as free(NULL))
        # ignore_case belongs to the set — said before anything else is looked at
        with pytest.raises(ValueError):
            res.select_device(sx.PatternSet(None), ignore_case=True)
        with pytest.raises(sx.SxError) as e:
            res.select_device(sx.PatternSet(None))                                           # a freed set
        assert e.value.code == sx.SX_E_INVALID
        # the list selection is where it was: 16 patterns of 64 bytes
        for bad in ([b"x"] * 17, [b"y" * 65]):
            with pytest.raises(sx.SxError) as e:
                res.select_device(bad)
            assert e.value.code == sx.SX_E_INVALID
        with pytest.raises(sx.SxError) as e:
            res.select_device([b"x"] * 16)
        assert e.value.code == sx.SX_E_STATE
        assert sx.SX_SELECT_MAX_PATTERNS == 16 and sx.SX_SELECT_MAX_PATTERN_BYTES == 64
        assert len(res.findings()) == len(res)                                               # the result is as good as before
        res.free()
    finally:
        sc.close()


def test_the_new_symbols_are_exported():
    for name in ("sx_select_set_create", "sx_select_set_info_get", "sx_select_set_free", "sx_result_select_set_device"):
        assert name in sx.EXPORTS and getattr(sx.lib(), name)
    assert sx.lib().sx_abi_version() == 4
    assert C.sizeof(sx.SelectSetInfo) == 32
