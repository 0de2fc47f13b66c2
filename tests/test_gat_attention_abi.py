"""Fused graph attention on A's pattern (sextans_gat_attention_device, sextans_gat_attention_backward_device): the symbols exist, bad
arguments and a handle without a matrix are refused with error codes before any device is touched (no GPU needed), and the Python
surfaces expose them."""
import ctypes as C
import inspect
import os

import pytest

from util import ROOT

OK = 0
INVALID = 9
STATE = 12

FWD = dict(heads=2, dv=16, slope=0.2, adst=16, ldadst=2, asrc=32, ldasrc=2, V=48, ldv=32, bias=0, O=64, ldo=32, lse=80)
BWD = dict(heads=2, dv=16, slope=0.2, adst=16, ldadst=2, asrc=32, ldasrc=2, V=48, ldv=32, bias=0, O=64, ldo=32, lse=80, G=96, ldg=32, delta=112,
           dadst=128, lddadst=2, dasrc=144, lddasrc=2, dV=160, lddv=32, dbias=0)

POINTERS = ("adst", "asrc", "V", "bias", "O", "lse", "G", "delta", "dadst", "dasrc", "dV", "dbias")   # passed as addresses: 0 = NULL


def call(L, name, h, base, **over):
    a = dict(base)
    a.update(over)
    return getattr(L, name)(h, *[(v or None) if k in POINTERS else v for k, v in a.items()], None)


# (name of the argument, value) -> SEXTANS_ERR_INVALID, on both entry points where the argument exists
BAD = [("heads", 0), ("heads", -1), ("dv", 0), ("dv", 12), ("dv", 136),
       ("slope", -0.1), ("slope", float("nan")), ("slope", float("inf")),
       ("ldadst", 1), ("ldasrc", 1), ("ldv", 31), ("ldv", 16), ("ldv", 38), ("ldo", 0), ("ldo", 35),
       ("adst", 20), ("asrc", 8), ("V", 4), ("bias", 24), ("O", 72), ("lse", 2)]
BAD_BWD = [("ldg", 24), ("ldg", 37), ("lddadst", 1), ("lddasrc", 0), ("lddv", 8), ("lddv", 34), ("G", 100), ("delta", 120), ("dadst", 132),
           ("dasrc", 12), ("dV", 168), ("dbias", 40)]


def test_symbols_exported(sx):
    from sextans_amd import api
    api.lib()
    raw = C.CDLL(api.LIB_PATH)
    for name in ("sextans_gat_attention_device", "sextans_gat_attention_backward_device"):
        assert name in api._OPTIONAL_SYMBOLS and hasattr(raw, name), name


@pytest.mark.parametrize("fake", [False, True])
def test_argument_checks(sx, fake):
    from sextans_amd import api
    L = api.lib()
    h = (C.c_char * (1 << 20))()   # a handle without a matrix (zeroed engine state)
    hp = C.addressof(h) if fake else None
    # a NULL handle is INVALID whatever else is passed; aligned, valid arguments on a handle without a CSR matrix: STATE, before any
    # device is touched
    want = STATE if fake else INVALID
    assert call(L, "sextans_gat_attention_device", hp, FWD) == want
    assert call(L, "sextans_gat_attention_backward_device", hp, BWD) == want
    assert call(L, "sextans_gat_attention_device", hp, FWD, bias=176) == want
    assert call(L, "sextans_gat_attention_backward_device", hp, BWD, bias=176, dbias=192) == want
    assert call(L, "sextans_gat_attention_device", hp, FWD, slope=0.0) == want
    assert call(L, "sextans_gat_attention_device", hp, FWD, slope=1.0, ldadst=3, ldasrc=7) == want   # any ld >= heads
    assert call(L, "sextans_gat_attention_device", hp, FWD, heads=1, dv=128, ldadst=1, ldasrc=1, ldv=128, ldo=132) == want
    assert call(L, "sextans_gat_attention_backward_device", hp, BWD, heads=1, dv=8, ldv=8, ldo=8, ldg=12, lddv=8, lddadst=5) == want
    for key, value in BAD:
        assert call(L, "sextans_gat_attention_device", hp, FWD, **{key: value}) == INVALID, (key, value)
        assert call(L, "sextans_gat_attention_backward_device", hp, BWD, **{key: value}) == INVALID, (key, value)
    for key, value in BAD_BWD:
        assert call(L, "sextans_gat_attention_backward_device", hp, BWD, **{key: value}) == INVALID, (key, value)


def test_python_and_torch_surfaces(sx):
    from sextans_amd import api, torch_op
    fwd = ["heads", "dv", "negative_slope", "d_adst", "ldadst", "d_asrc", "ldasrc", "d_V", "ldv", "d_bias", "d_O", "ldo", "d_lse", "stream"]
    bwd = ["heads", "dv", "negative_slope", "d_adst", "ldadst", "d_asrc", "ldasrc", "d_V", "ldv", "d_bias", "d_O", "ldo", "d_lse", "d_G", "ldg",
           "d_delta", "d_dadst", "lddadst", "d_dasrc", "lddasrc", "d_dV", "lddv", "d_dbias", "stream"]
    for name, params in (("gat_attention_device", fwd), ("gat_attention_backward_device", bwd)):
        sig = inspect.signature(getattr(api.Engine, name)).parameters
        assert list(sig)[1:] == params, name
        assert sig["stream"].default is None
    sig = inspect.signature(torch_op.gat_attention).parameters
    assert list(sig) == ["A", "a_dst", "a_src", "V", "negative_slope", "bias", "fast"]
    assert sig["negative_slope"].default == 0.2 and sig["bias"].default is False and sig["fast"].default is False
    with open(os.path.join(ROOT, "include", "sextans_amd.h")) as f:
        text = " ".join(f.read().split())
    assert ("int sextans_gat_attention_device(sextans_handle_t h, int heads, int dv, float negative_slope, const float *d_adst, int64_t ldadst, "
            "const float *d_asrc, int64_t ldasrc, const float *d_V, int64_t ldv, const float *d_bias, float *d_O, int64_t ldo, float *d_lse, "
            "void *stream);") in text
    assert ("int sextans_gat_attention_backward_device(sextans_handle_t h, int heads, int dv, float negative_slope, const float *d_adst, "
            "int64_t ldadst, const float *d_asrc, int64_t ldasrc, const float *d_V, int64_t ldv, const float *d_bias, const float *d_O, "
            "int64_t ldo, const float *d_lse, const float *d_G, int64_t ldg, float *d_delta, float *d_dadst, int64_t lddadst, "
            "float *d_dasrc, int64_t lddasrc, float *d_dV, int64_t lddv, float *d_dbias, void *stream);") in text
