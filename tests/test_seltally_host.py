"""sx_tally_set_create and sx_result_tally_device without a GPU: a host-only context has no device for a set's tables and no
device-resident result, so both are refused with SX_E_STATE; bad arguments are SX_E_INVALID, told apart from that."""
import ctypes as C
import random

import pytest

import refconfig as rc
import stringsext_amd as sx
from product_harness import oracle_runs_for_chunk
from test_host_logic import synth

NAMES = ("sx_tally_set_create", "sx_tally_set_info_get", "sx_tally_set_free", "sx_tally_set_reset", "sx_result_tally_device",
         "sx_tally_set_read", "sx_tally_set_counters_device")


def test_the_new_symbols_are_exported_and_the_abi_version_stays():
    for name in NAMES:
        assert name in sx.EXPORTS and getattr(sx.lib(), name)
    assert sx.lib().sx_abi_version() == 4
    assert C.sizeof(sx.TallySetInfo) == 40
    assert sx.SX_TALLY_NEVER == 2 ** 64 - 1


def create_rc(sc, patterns, n=None, flags=0):
    arr = (sx.Pattern * max(1, len(patterns)))(*[sx.Pattern(p, ln) for p, ln in patterns])
    out = C.c_void_p(1)
    code = sx.lib().sx_tally_set_create(sc.h, arr, len(patterns) if n is None else n, flags, C.byref(out))
    assert code != sx.SX_OK and out.value is None          # *out = NULL on every error
    return code


def test_a_host_only_context_is_refused_and_bad_arguments_are_invalid():
    L = sx.lib()
    rng = random.Random(2028)
    data = synth(rng, 300_000, 1 / 300)
    ms = rc.missions(encodings=["utf-8", "utf-16le"], chars_min="10")
    sc = sx.Scanner(ms, device=sx.SX_HOST_ONLY, result_on_device=True)
    try:
        res = sc.replay_runs(data, oracle_runs_for_chunk(ms, data, 0), file_id=1)
        assert len(res) > 10
        # a set that could be built has no device to lie on
        for kw in (dict(), dict(ignore_case=True)):
            with pytest.raises(sx.SxError) as e:
                sc.tally_set([b"abc", b"de", b"abc"], **kw)
            assert e.value.code == sx.SX_E_STATE
        assert create_rc(sc, [(b"abc", 3)]) == sx.SX_E_STATE
        assert create_rc(sc, [(b"q" * 255, 255)] * 4112 + [(b"q" * 16, 16)]) == sx.SX_E_STATE      # 1 MiB in all
        # every SX_E_INVALID case of create is told apart from that
        for bad in ([], [b""], [b"ok", b""], [b"y" * 256], [b"q" * 255] * 4112 + [b"q" * 17]):
            with pytest.raises(sx.SxError) as e:
                sc.tally_set(bad)
            assert e.value.code == sx.SX_E_INVALID, bad[:2]
        assert create_rc(sc, [(b"abc", 3)], n=0) == sx.SX_E_INVALID
        assert create_rc(sc, [(b"abc", 3)] * 2, n=65537) == sx.SX_E_INVALID                 # (refused before a pattern is read)
        assert create_rc(sc, [(b"abc", 0)]) == sx.SX_E_INVALID
        assert create_rc(sc, [(b"y" * 256, 256)]) == sx.SX_E_INVALID
        assert create_rc(sc, [(b"abc", 3)], flags=sx.SX_SELECT_INVERT) == sx.SX_E_INVALID   # a foreign flag bit
        assert create_rc(sc, [(b"abc", 3)], flags=4) == sx.SX_E_INVALID
        assert create_rc(sc, [(b"abc", 3)], flags=1 | 1 << 31) == sx.SX_E_INVALID
        assert create_rc(sc, [(None, 3)]) == sx.SX_E_INVALID                                # a NULL pattern
        out = C.c_void_p(1)
        assert L.sx_tally_set_create(sc.h, None, 1, 0, C.byref(out)) == sx.SX_E_INVALID and out.value is None
        arr = (sx.Pattern * 1)(sx.Pattern(b"abc", 3))
        assert L.sx_tally_set_create(sc.h, arr, 1, 0, None) == sx.SX_E_INVALID
        assert L.sx_tally_set_create(None, arr, 1, 0, C.byref(out)) == sx.SX_E_INVALID and out.value is None
        # NULL sets (no set can exist here)
        L.sx_tally_set_free(None)                                                            # (as free(NULL))
        info = sx.TallySetInfo()
        assert L.sx_tally_set_info_get(None, C.byref(info)) == sx.SX_E_INVALID
        hits = (C.c_uint64 * 1)()
        assert L.sx_tally_set_read(None, hits, hits, 1) == sx.SX_E_INVALID
        assert L.sx_tally_set_reset(None) == sx.SX_E_INVALID
        assert L.sx_tally_set_counters_device(None, None, None, None, None) == sx.SX_E_INVALID
        n = C.c_uint64(7)
        assert L.sx_result_tally_device(sc.h, res.h, None, 0, C.byref(n)) == sx.SX_E_INVALID and n.value == 0
        assert L.sx_result_tally_device(None, res.h, None, 0, None) == sx.SX_E_INVALID
        # a freed TallySet is said to be one before anything is called
        gone = sx.TallySet(None, 1)
        for call in (gone.info, gone.read, gone.reset, gone.counters_device, lambda: res.tally_device(gone)):
            with pytest.raises(sx.SxError) as e:
                call()
            assert e.value.code == sx.SX_E_INVALID
        gone.free(); gone.free()                                                             # (twice is once)
        assert len(res.findings()) == len(res)                                               # the result is as good as before
        res.free()
    finally:
        sc.close()
