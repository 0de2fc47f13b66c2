"""Edge-output ops from both endpoints (sextans_edge_op_device_rm, sextans_edge_op_backward_device_rm): the symbols exist, bad arguments
and a handle without a matrix are refused with error codes before any device is touched, in the order the header states (no GPU needed),
and the Python surfaces expose them."""
import ctypes as C
import inspect
import os

import pytest

from util import ROOT

OK = 0
INVALID = 9
STATE = 12

ADD, SUB, MUL, DST, SRC = 1, 2, 3, 4, 5
OPS = (ADD, SUB, MUL, DST, SRC)

FWD = dict(op=ADD, N=16, xdst=16, ldxdst=16, xsrc=32, ldxsrc=16, E=48, lde=16, Z=64, ldz=16)
BWD = dict(op=MUL, N=16, xdst=16, ldxdst=16, xsrc=32, ldxsrc=16, Gz=48, ldgz=16, dxdst=64, lddxdst=16, dxsrc=80, lddxsrc=16)

POINTERS = ("xdst", "xsrc", "E", "Z", "Gz", "dxdst", "dxsrc")   # passed as addresses: 0 = NULL

FWD_NAME, BWD_NAME = "sextans_edge_op_device_rm", "sextans_edge_op_backward_device_rm"

# the gradients an op has no operand for must not be asked for
NOT_OF = {ADD: {}, SUB: {}, MUL: {}, DST: dict(dxsrc=0), SRC: dict(dxdst=0)}


def call(L, name, h, base, **over):
    a = dict(base)
    a.update(over)
    return getattr(L, name)(h, *[(v or None) if k in POINTERS else v for k, v in a.items()], None)


# (name of the argument, value) -> SEXTANS_ERR_INVALID on both entry points: ADD reads both operands in the forward, MUL with both
# gradients reads both in the backward
BAD = [("op", 0), ("op", 6), ("op", -1), ("N", 0), ("N", 4), ("N", 12), ("N", -8), ("ldxdst", 8), ("ldxdst", 18), ("ldxsrc", 12),
       ("ldxsrc", 17), ("xdst", 24), ("xsrc", 36)]
BAD_FWD = [("lde", 8), ("lde", 21), ("ldz", 0), ("ldz", 22), ("E", 52), ("Z", 68)]
BAD_BWD = [("ldgz", 15), ("ldgz", 18), ("lddxdst", 8), ("lddxdst", 21), ("lddxsrc", 12), ("lddxsrc", 22), ("Gz", 56), ("dxdst", 68),
           ("dxsrc", 88)]


def test_symbols_exported(sx):
    from sextans_amd import api
    api.lib()
    raw = C.CDLL(api.LIB_PATH)
    for name in (FWD_NAME, BWD_NAME):
        assert name in api._OPTIONAL_SYMBOLS and hasattr(raw, name), name
    assert (api.EDGEOP_ADD, api.EDGEOP_SUB, api.EDGEOP_MUL, api.EDGEOP_DST, api.EDGEOP_SRC) == OPS


@pytest.mark.parametrize("fake", [False, True])
def test_argument_checks(sx, fake):
    from sextans_amd import api
    L = api.lib()
    h = (C.c_char * (1 << 20))()   # a handle without a matrix (zeroed engine state)
    hp = C.addressof(h) if fake else None
    # a NULL handle is INVALID whatever else is passed; aligned, valid arguments on a handle without a CSR matrix: STATE, before any
    # device is touched
    want = STATE if fake else INVALID
    for op in OPS:
        no = NOT_OF[op]
        assert call(L, FWD_NAME, hp, FWD, op=op) == want
        assert call(L, BWD_NAME, hp, BWD, op=op, **no) == want
        assert call(L, FWD_NAME, hp, FWD, op=op, ldxdst=20, ldxsrc=24, lde=32, ldz=28) == want        # any ld >= N that is a multiple of 4
        assert call(L, BWD_NAME, hp, BWD, op=op, ldxdst=20, ldxsrc=24, ldgz=28, lddxdst=32, lddxsrc=20, **no) == want
        assert call(L, FWD_NAME, hp, FWD, op=op, E=0) == want                                          # no edge features ...
        assert call(L, FWD_NAME, hp, FWD, op=op, E=0, lde=3) == want                                   # ... and then lde is not looked at
        assert call(L, FWD_NAME, hp, FWD, op=op, N=264, ldxdst=264, ldxsrc=272, lde=264, ldz=268) == want   # N has no upper limit
        assert call(L, BWD_NAME, hp, BWD, op=op, N=264, ldxdst=264, ldxsrc=272, ldgz=264, lddxdst=268, lddxsrc=264, **no) == want
        assert call(L, BWD_NAME, hp, BWD, op=op, dxdst=0, dxsrc=0) == INVALID                          # nothing to compute
        # each gradient alone where the op has it; the leading dimension of an absent gradient is ignored
        if op != SRC:
            assert call(L, BWD_NAME, hp, BWD, op=op, dxsrc=0) == want
            assert call(L, BWD_NAME, hp, BWD, op=op, dxsrc=0, lddxsrc=3) == want
        if op != DST:
            assert call(L, BWD_NAME, hp, BWD, op=op, dxdst=0) == want
            assert call(L, BWD_NAME, hp, BWD, op=op, dxdst=0, lddxdst=0) == want
    # an operand the op does not read is ignored: absent, misaligned or with any leading dimension
    assert call(L, FWD_NAME, hp, FWD, op=DST, xsrc=0, ldxsrc=0) == want
    assert call(L, FWD_NAME, hp, FWD, op=DST, xsrc=36, ldxsrc=3) == want
    assert call(L, FWD_NAME, hp, FWD, op=SRC, xdst=0, ldxdst=0) == want
    assert call(L, FWD_NAME, hp, FWD, op=SRC, xdst=20, ldxdst=5) == want
    assert call(L, FWD_NAME, hp, FWD, op=DST, ldxdst=8) == INVALID   # (one it reads counts)
    assert call(L, FWD_NAME, hp, FWD, op=SRC, ldxsrc=8) == INVALID
    # the backward reads an endpoint only for MUL, and then the OTHER endpoint of a gradient that is asked for
    for op in (ADD, SUB, DST, SRC):
        assert call(L, BWD_NAME, hp, BWD, op=op, xdst=0, ldxdst=0, xsrc=0, ldxsrc=0, **NOT_OF[op]) == want
        assert call(L, BWD_NAME, hp, BWD, op=op, xdst=20, ldxdst=3, xsrc=36, ldxsrc=5, **NOT_OF[op]) == want
    assert call(L, BWD_NAME, hp, BWD, op=MUL, dxsrc=0, xdst=0, ldxdst=0) == want     # dxdst alone reads xsrc only
    assert call(L, BWD_NAME, hp, BWD, op=MUL, dxsrc=0, xdst=20, ldxdst=3) == want
    assert call(L, BWD_NAME, hp, BWD, op=MUL, dxdst=0, xsrc=0, ldxsrc=0) == want     # dxsrc alone reads xdst only
    assert call(L, BWD_NAME, hp, BWD, op=MUL, dxdst=0, xsrc=36, ldxsrc=3) == want
    assert call(L, BWD_NAME, hp, BWD, op=MUL, dxsrc=0, ldxsrc=8) == INVALID
    assert call(L, BWD_NAME, hp, BWD, op=MUL, dxdst=0, ldxdst=8) == INVALID
    # a gradient of an operand the op does not read is refused -- before the handle's state is looked at
    assert call(L, BWD_NAME, hp, BWD, op=DST) == INVALID
    assert call(L, BWD_NAME, hp, BWD, op=DST, dxdst=0) == INVALID
    assert call(L, BWD_NAME, hp, BWD, op=SRC) == INVALID
    assert call(L, BWD_NAME, hp, BWD, op=SRC, dxsrc=0) == INVALID
    # a required pointer that is NULL comes after the state: STATE on the fake handle, not INVALID
    for key in ("xdst", "xsrc", "Z"):
        assert call(L, FWD_NAME, hp, FWD, **{key: 0}) == want, key
    for key in ("xdst", "xsrc", "Gz"):
        assert call(L, BWD_NAME, hp, BWD, **{key: 0}) == want, key
    for key, value in BAD:
        assert call(L, FWD_NAME, hp, FWD, **{key: value}) == INVALID, (key, value)
        assert call(L, BWD_NAME, hp, BWD, **{key: value}) == INVALID, (key, value)
    for key, value in BAD_FWD:
        assert call(L, FWD_NAME, hp, FWD, **{key: value}) == INVALID, (key, value)
    for key, value in BAD_BWD:
        assert call(L, BWD_NAME, hp, BWD, **{key: value}) == INVALID, (key, value)
    # more column tiles than the long-row kernel's grid has (65535 of 128 floats); the largest N that fits is not refused for its size
    big = 65536 * 128
    assert call(L, FWD_NAME, hp, FWD, N=big, ldxdst=big, ldxsrc=big, lde=big, ldz=big) == INVALID
    assert call(L, BWD_NAME, hp, BWD, N=big, ldxdst=big, ldxsrc=big, ldgz=big, lddxdst=big, lddxsrc=big) == INVALID
    most = 65535 * 128
    assert call(L, FWD_NAME, hp, FWD, N=most, ldxdst=most, ldxsrc=most, lde=most, ldz=most) == want
    assert call(L, BWD_NAME, hp, BWD, N=most, ldxdst=most, ldxsrc=most, ldgz=most, lddxdst=most, lddxsrc=most) == want


def test_python_and_torch_surfaces(sx):
    from sextans_amd import api, edge_op, torch_op
    fwd = ["op", "N", "d_xdst", "ldxdst", "d_xsrc", "ldxsrc", "d_E", "lde", "d_Z", "ldz", "stream"]
    bwd = ["op", "N", "d_xdst", "ldxdst", "d_xsrc", "ldxsrc", "d_Gz", "ldgz", "d_dxdst", "lddxdst", "d_dxsrc", "lddxsrc", "stream"]
    for name, params in (("edge_op_device_rm", fwd), ("edge_op_backward_device_rm", bwd)):
        sig = inspect.signature(getattr(api.Engine, name)).parameters
        assert list(sig)[1:] == params, name
        assert sig["stream"].default is None
    sig = inspect.signature(edge_op.edge_op).parameters
    assert list(sig) == ["A", "x_dst", "x_src", "E", "op", "fast"]
    assert sig["x_dst"].default is None and sig["x_src"].default is None and sig["E"].default is None
    assert sig["op"].default == "add" and sig["fast"].default is False
    assert edge_op.__all__ == ["edge_op"]
    assert not hasattr(torch_op, "edge_op") and "sextans_amd.edge_op" in torch_op.__doc__
    with open(os.path.join(ROOT, "include", "sextans_amd.h")) as f:
        text = " ".join(f.read().split())
    assert ("int sextans_edge_op_device_rm(sextans_handle_t h, int op, int N, const float *d_xdst, int64_t ldxdst, const float *d_xsrc, "
            "int64_t ldxsrc, const float *d_E, int64_t lde, float *d_Z, int64_t ldz, void *stream);") in text
    assert ("int sextans_edge_op_backward_device_rm(sextans_handle_t h, int op, int N, const float *d_xdst, int64_t ldxdst, "
            "const float *d_xsrc, int64_t ldxsrc, const float *d_Gz, int64_t ldgz, float *d_dxdst, int64_t lddxdst, float *d_dxsrc, "
            "int64_t lddxsrc, void *stream);") in text
    for name in ("SEXTANS_EDGEOP_ADD 1", "SEXTANS_EDGEOP_SUB 2", "SEXTANS_EDGEOP_MUL 3", "SEXTANS_EDGEOP_DST 4", "SEXTANS_EDGEOP_SRC 5"):
        assert "#define " + name in text
