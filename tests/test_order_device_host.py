"""sx_result_order_device without a GPU: a host-only context has no device-resident result, so the call is refused with SX_E_STATE
(the caller sorts on the host); bad arguments are SX_E_INVALID, told apart from that and decided first."""
import ctypes as C
import random

import pytest

import refconfig as rc
import stringsext_amd as sx
from product_harness import oracle_runs_for_chunk
from test_host_logic import synth


def order_rc(sc, res, labels=None, with_spec=True, with_out=True, **spec):
    s = sx.OrderSpec(spec.get("by", sx.SX_ORDER_BY_STRING), spec.get("flags", 0), spec.get("shift", 0), spec.get("bits", 64),
                     spec.get("any", 0), spec.get("all", 0), spec.get("none", 0), spec.get("limit", 0))
    out, info = C.c_void_p(1), sx.OrderInfo()
    code = sx.lib().sx_result_order_device(sc.h if sc else None, res.h if res else None, labels, C.byref(s) if with_spec else None,
                                           C.byref(out) if with_out else None, C.byref(info))
    assert not with_out or out.value is None          # *out = NULL on every error
    return code


def test_a_host_only_context_is_refused_and_bad_arguments_are_invalid():
    data = synth(random.Random(2027), 300_000, 1 / 300)
    ms = rc.missions(encodings=["utf-8", "utf-16le"], chars_min="10")
    sc = sx.Scanner(ms, device=sx.SX_HOST_ONLY, result_on_device=True)
    try:
        res = sc.replay_runs(data, oracle_runs_for_chunk(ms, data, 0), file_id=1)
        assert len(res) > 10
        F, D, N = sx.SX_ORDER_BY_LABEL_FIELD, sx.SX_ORDER_DESCENDING, sx.SX_ORDER_NOCASE
        # a call without fault: there is no device
        for spec in (dict(), dict(flags=D), dict(flags=N), dict(flags=D | N, limit=20)):
            assert order_rc(sc, res, **spec) == sx.SX_E_STATE, spec
            assert "host-only" in sx.lib().sx_last_error(sc.h).decode()
        for kw in (dict(), dict(descending=True, ignore_case=True, limit=3)):
            with pytest.raises(sx.SxError) as e:
                res.order_device(**kw)
            assert e.value.code == sx.SX_E_STATE
        # bad arguments are told apart from a result that is in the wrong place
        invalid = [dict(by=2), dict(by=1 << 31), dict(flags=4), dict(flags=3 | 1 << 31),          # an unknown key, an unknown flag
                   dict(by=F, flags=N, shift=32, bits=32),                                            # the fold with the label key (and no labels)
                   dict(by=F, shift=32, bits=32), dict(by=F, shift=0, bits=64),                       # the label key without labels
                   dict(any=1), dict(all=2), dict(none=4), dict(flags=D, any=1, limit=5),             # a filter without labels
                   dict(by=F, bits=0), dict(by=F, bits=65), dict(by=F, shift=33, bits=32), dict(by=F, shift=64, bits=1)]      # a field select_range refuses
        for spec in invalid:
            assert order_rc(sc, res, **spec) == sx.SX_E_INVALID, spec
            assert sx.lib().sx_last_error(sc.h).decode().startswith("order: "), spec
        assert order_rc(None, res) == sx.SX_E_INVALID and order_rc(sc, None) == sx.SX_E_INVALID
        assert order_rc(sc, res, with_spec=False) == sx.SX_E_INVALID and order_rc(sc, res, with_out=False) == sx.SX_E_INVALID
        for kw in (dict(by="field"), dict(by="field", shift=40, bits=32), dict(any=1), dict(by="field", ignore_case=True)):
            with pytest.raises(sx.SxError) as e:
                res.order_device(**kw)
            assert e.value.code == sx.SX_E_INVALID, kw
        with pytest.raises(ValueError):
            res.order_device(by="position")
        with pytest.raises(TypeError):
            res.order_device(labels=object())
        assert (sx.SX_ORDER_BY_STRING, sx.SX_ORDER_BY_LABEL_FIELD, sx.SX_ORDER_DESCENDING, sx.SX_ORDER_NOCASE) == (0, 1, 1, 2)
        assert C.sizeof(sx.OrderSpec) == 48 and C.sizeof(sx.OrderInfo) == 40
        # the result is as good as before
        assert len(res.findings()) == len(res)
        res.free()
    finally:
        sc.close()
    with pytest.raises(sx.SxError) as e:      # a closed Scanner
        sx.Result(sc, None).order_device()
    assert e.value.code == sx.SX_E_STATE
