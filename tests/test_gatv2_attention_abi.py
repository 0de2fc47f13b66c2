"""Fused GATv2 attention on A's pattern (sextans_gatv2_workspace_floats, sextans_gatv2_attention_device,
sextans_gatv2_attention_backward_device): the symbols exist, bad arguments and a handle without a matrix are refused with error codes
before any device is touched (no GPU needed), and the Python surfaces expose them."""
import ctypes as C
import inspect
import os

import pytest

from util import ROOT

OK = 0
INVALID = 9
STATE = 12

FWD = dict(heads=2, d=16, slope=0.2, xdst=16, ldxd=32, xsrc=32, ldxs=32, att=48, bias=0, O=64, ldo=32, lse=80)
BWD = dict(heads=2, d=16, slope=0.2, xdst=16, ldxd=32, xsrc=32, ldxs=32, att=48, bias=0, O=64, ldo=32, lse=80, G=96, ldg=32, delta=112,
           dxdst=128, lddxd=32, dxsrc=144, lddxs=32, datt=160, work=176, dbias=0)

POINTERS = ("xdst", "xsrc", "att", "bias", "O", "lse", "G", "delta", "dxdst", "dxsrc", "datt", "work", "dbias")   # passed as addresses: 0 = NULL


def call(L, name, h, base, **over):
    a = dict(base)
    a.update(over)
    return getattr(L, name)(h, *[(v or None) if k in POINTERS else v for k, v in a.items()], None)


# (name of the argument, value) -> SEXTANS_ERR_INVALID, on both entry points where the argument exists
BAD = [("heads", 0), ("heads", -1), ("d", 0), ("d", 12), ("d", 136),
       ("slope", -0.1), ("slope", float("nan")), ("slope", float("inf")),
       ("ldxd", 31), ("ldxd", 16), ("ldxd", 38), ("ldxs", 0), ("ldxs", 35), ("ldo", 28), ("ldo", 33),
       ("xdst", 20), ("xsrc", 8), ("att", 4), ("bias", 24), ("O", 72), ("lse", 2)]
BAD_BWD = [("ldg", 24), ("ldg", 37), ("lddxd", 16), ("lddxd", 34), ("lddxs", 8), ("lddxs", 39), ("G", 100), ("delta", 120), ("dxdst", 132),
           ("dxsrc", 12), ("datt", 168), ("work", 180), ("dbias", 40)]
NAMES = ("sextans_gatv2_workspace_floats", "sextans_gatv2_attention_device", "sextans_gatv2_attention_backward_device")


def test_symbols_exported(sx):
    from sextans_amd import api
    api.lib()
    raw = C.CDLL(api.LIB_PATH)
    for name in NAMES:
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
    fwd, bwd = "sextans_gatv2_attention_device", "sextans_gatv2_attention_backward_device"
    assert call(L, fwd, hp, FWD) == want
    assert call(L, bwd, hp, BWD) == want
    assert call(L, fwd, hp, FWD, bias=192) == want
    assert call(L, bwd, hp, BWD, bias=192, dbias=208) == want
    assert call(L, fwd, hp, FWD, slope=0.0) == want
    assert call(L, fwd, hp, FWD, slope=1.0, ldxd=36, ldxs=64) == want   # any ld >= heads * d that is a multiple of 4
    assert call(L, fwd, hp, FWD, xsrc=16) == want                       # x_dst and x_src may be one array
    assert call(L, fwd, hp, FWD, heads=1, d=128, ldxd=128, ldxs=128, ldo=132) == want
    assert call(L, bwd, hp, BWD, heads=1, d=8, ldxd=8, ldxs=8, ldo=8, ldg=12, lddxd=8, lddxs=20) == want
    for key, value in BAD:
        assert call(L, fwd, hp, FWD, **{key: value}) == INVALID, (key, value)
        assert call(L, bwd, hp, BWD, **{key: value}) == INVALID, (key, value)
    for key, value in BAD_BWD:
        assert call(L, bwd, hp, BWD, **{key: value}) == INVALID, (key, value)
    # the workspace query returns the error code negated
    ws = L.sextans_gatv2_workspace_floats
    assert ws.restype is C.c_int64
    assert ws(hp, 2, 16) == -want
    for heads, d in ((0, 16), (-1, 16), (2, 0), (2, 12), (2, 136)):
        assert ws(hp, heads, d) == -INVALID, (heads, d)


def test_python_and_torch_surfaces(sx):
    from sextans_amd import api, torch_op
    fwd = ["heads", "d", "negative_slope", "d_xdst", "ldxd", "d_xsrc", "ldxs", "d_att", "d_bias", "d_O", "ldo", "d_lse", "stream"]
    bwd = ["heads", "d", "negative_slope", "d_xdst", "ldxd", "d_xsrc", "ldxs", "d_att", "d_bias", "d_O", "ldo", "d_lse", "d_G", "ldg",
           "d_delta", "d_dxdst", "lddxd", "d_dxsrc", "lddxs", "d_datt", "d_work", "d_dbias", "stream"]
    for name, params in (("gatv2_attention_device", fwd), ("gatv2_attention_backward_device", bwd)):
        sig = inspect.signature(getattr(api.Engine, name)).parameters
        assert list(sig)[1:] == params, name
        assert sig["stream"].default is None
    assert list(inspect.signature(api.Engine.gatv2_workspace_floats).parameters)[1:] == ["heads", "d"]
    sig = inspect.signature(torch_op.gatv2_attention).parameters
    assert list(sig) == ["A", "x_dst", "x_src", "att", "negative_slope", "bias", "fast"]
    assert sig["negative_slope"].default == 0.2 and sig["bias"].default is False and sig["fast"].default is False
    with open(os.path.join(ROOT, "include", "sextans_amd.h")) as f:
        text = " ".join(f.read().split())
    assert "int64_t sextans_gatv2_workspace_floats(sextans_handle_t h, int heads, int d);" in text
    assert ("int sextans_gatv2_attention_device(sextans_handle_t h, int heads, int d, float negative_slope, const float *d_xdst, int64_t ldxd, "
            "const float *d_xsrc, int64_t ldxs, const float *d_att, const float *d_bias, float *d_O, int64_t ldo, float *d_lse, "
            "void *stream);") in text
    assert ("int sextans_gatv2_attention_backward_device(sextans_handle_t h, int heads, int d, float negative_slope, const float *d_xdst, "
            "int64_t ldxd, const float *d_xsrc, int64_t ldxs, const float *d_att, const float *d_bias, const float *d_O, int64_t ldo, "
            "const float *d_lse, const float *d_G, int64_t ldg, float *d_delta, float *d_dxdst, int64_t lddxd, float *d_dxsrc, "
            "int64_t lddxs, float *d_datt, float *d_work, float *d_dbias, void *stream);") in text
