"""Per-head dot product on the pattern (sextans_edge_dot_device, sextans_edge_dot_backward_device): the symbols exist, bad arguments and a
handle without a matrix are refused with error codes before any device is touched, in the order the header states (no GPU needed), and
the Python surfaces expose them."""
import ctypes as C
import inspect
import os

import pytest

from util import ROOT

OK = 0
INVALID = 9
STATE = 12

# heads = 3, d = 16: a row of X, Y, dX, dY holds 48 floats
FWD = dict(heads=3, d=16, X=16, ldx=48, Y=32, ldy=48, S=48, lds=3)
BWD = dict(heads=3, d=16, X=16, ldx=48, Y=32, ldy=48, Gs=48, ldgs=3, dX=64, lddx=48, dY=80, lddy=48)

POINTERS = ("X", "Y", "S", "Gs", "dX", "dY")   # passed as addresses: 0 = NULL

FWD_NAME, BWD_NAME = "sextans_edge_dot_device", "sextans_edge_dot_backward_device"


def call(L, name, h, base, **over):
    a = dict(base)
    a.update(over)
    return getattr(L, name)(h, *[(v or None) if k in POINTERS else v for k, v in a.items()], None)


# (name of the argument, value) -> SEXTANS_ERR_INVALID on both entry points (the backward with both gradients reads X and Y)
BAD = [("heads", 0), ("heads", -1), ("heads", 65536), ("d", 0), ("d", 4), ("d", 12), ("d", 136), ("d", -8), ("ldx", 40), ("ldx", 47), ("ldx", 50),
       ("ldy", 16), ("ldy", 49), ("X", 24), ("Y", 36)]
BAD_FWD = [("lds", 2), ("lds", 0), ("S", 52)]
BAD_BWD = [("ldgs", 2), ("ldgs", 0), ("lddx", 44), ("lddx", 50), ("lddy", 32), ("lddy", 51), ("Gs", 56), ("dX", 68), ("dY", 88)]


def test_symbols_exported(sx):
    from sextans_amd import api
    api.lib()
    raw = C.CDLL(api.LIB_PATH)
    for name in (FWD_NAME, BWD_NAME):
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
    assert call(L, FWD_NAME, hp, FWD) == want
    assert call(L, BWD_NAME, hp, BWD) == want
    for heads, d in ((1, 8), (1, 128), (8, 64), (65535, 8)):
        n = heads * d
        assert call(L, FWD_NAME, hp, FWD, heads=heads, d=d, ldx=n, ldy=n + 4, lds=heads) == want
        assert call(L, BWD_NAME, hp, BWD, heads=heads, d=d, ldx=n, ldy=n + 4, ldgs=heads, lddx=n + 8, lddy=n) == want
    # any ldx, ldy >= heads * d that is a multiple of 4; lds, ldgs >= heads, whatever their remainder
    assert call(L, FWD_NAME, hp, FWD, ldx=52, ldy=64, lds=5) == want
    assert call(L, BWD_NAME, hp, BWD, ldx=52, ldy=64, ldgs=7, lddx=56, lddy=60) == want
    # nothing to compute -- before the handle's state is looked at
    assert call(L, BWD_NAME, hp, BWD, dX=0, dY=0) == INVALID
    # each gradient alone; the leading dimension of an absent gradient is ignored
    assert call(L, BWD_NAME, hp, BWD, dY=0) == want
    assert call(L, BWD_NAME, hp, BWD, dY=0, lddy=3) == want
    assert call(L, BWD_NAME, hp, BWD, dX=0) == want
    assert call(L, BWD_NAME, hp, BWD, dX=0, lddx=0) == want
    # X is read only for dY and Y only for dX: the one a call does not read is ignored -- absent, misaligned or with any leading dimension
    assert call(L, BWD_NAME, hp, BWD, dY=0, X=0, ldx=0) == want
    assert call(L, BWD_NAME, hp, BWD, dY=0, X=20, ldx=3) == want
    assert call(L, BWD_NAME, hp, BWD, dX=0, Y=0, ldy=0) == want
    assert call(L, BWD_NAME, hp, BWD, dX=0, Y=36, ldy=5) == want
    assert call(L, BWD_NAME, hp, BWD, dY=0, ldy=40) == INVALID   # (the one it reads counts)
    assert call(L, BWD_NAME, hp, BWD, dX=0, ldx=40) == INVALID
    assert call(L, BWD_NAME, hp, BWD, dY=0, Y=36) == INVALID
    assert call(L, BWD_NAME, hp, BWD, dX=0, X=20) == INVALID
    # a required pointer that is NULL comes after the state: STATE on the fake handle, not INVALID
    for key in ("X", "Y", "S"):
        assert call(L, FWD_NAME, hp, FWD, **{key: 0}) == want, key
    for key in ("X", "Y", "Gs"):
        assert call(L, BWD_NAME, hp, BWD, **{key: 0}) == want, key
    for key, value in BAD:
        assert call(L, FWD_NAME, hp, FWD, **{key: value}) == INVALID, (key, value)
        assert call(L, BWD_NAME, hp, BWD, **{key: value}) == INVALID, (key, value)
    for key, value in BAD_FWD:
        assert call(L, FWD_NAME, hp, FWD, **{key: value}) == INVALID, (key, value)
    for key, value in BAD_BWD:
        assert call(L, BWD_NAME, hp, BWD, **{key: value}) == INVALID, (key, value)
    # the order of the header, where codes tell it: every argument check comes BEFORE the state (INVALID on the fake handle too, even
    # with a required pointer NULL as well), a NULL operand alone after it (above)
    assert call(L, FWD_NAME, hp, FWD, heads=0, X=0) == INVALID
    assert call(L, FWD_NAME, hp, FWD, X=24, Y=0) == INVALID
    assert call(L, BWD_NAME, hp, BWD, dX=0, dY=0, Gs=0) == INVALID


def test_python_and_torch_surfaces(sx):
    from sextans_amd import api, edge_dot, edge_op, torch_op
    fwd = ["heads", "d", "d_X", "ldx", "d_Y", "ldy", "d_S", "lds", "stream"]
    bwd = ["heads", "d", "d_X", "ldx", "d_Y", "ldy", "d_Gs", "ldgs", "d_dX", "lddx", "d_dY", "lddy", "stream"]
    for name, params in (("edge_dot_device", fwd), ("edge_dot_backward_device", bwd)):
        sig = inspect.signature(getattr(api.Engine, name)).parameters
        assert list(sig)[1:] == params, name
        assert sig["stream"].default is None
    sig = inspect.signature(edge_dot.edge_dot).parameters
    assert list(sig) == ["A", "x_dst", "x_src", "fast"]
    assert sig["fast"].default is False
    assert edge_dot.__all__ == ["edge_dot"]
    assert edge_op.__all__ == ["edge_op"] and not hasattr(torch_op, "edge_dot")   # the pinned surfaces stay as they are
    with open(os.path.join(ROOT, "include", "sextans_amd.h")) as f:
        text = " ".join(f.read().split())
    assert ("int sextans_edge_dot_device(sextans_handle_t h, int heads, int d, const float *d_X, int64_t ldx, const float *d_Y, int64_t ldy, "
            "float *d_S, int64_t lds, void *stream);") in text
    assert ("int sextans_edge_dot_backward_device(sextans_handle_t h, int heads, int d, const float *d_X, int64_t ldx, const float *d_Y, "
            "int64_t ldy, const float *d_Gs, int64_t ldgs, float *d_dX, int64_t lddx, float *d_dY, int64_t lddy, void *stream);") in text
