"""SpMM with a feature vector per entry (sextans_spmm_edge_device_rm, sextans_spmm_edge_backward_device_rm): the symbols exist, bad
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
MUL, ADD, ADD_RELU, COPY = 1, 2, 3, 4

FWD = dict(op=1, N=16, B=32, ldb=16, E=48, lde=16, C=64, ldc=16)
BWD = dict(op=1, N=16, B=32, ldb=16, E=48, lde=16, G=80, ldg=16, dB=96, lddb=16, dE=112, ldde=16)

POINTERS = ("B", "E", "C", "G", "dB", "dE")   # passed as addresses: 0 = NULL

FWD_NAME, BWD_NAME = "sextans_spmm_edge_device_rm", "sextans_spmm_edge_backward_device_rm"


def call(L, name, h, base, **over):
    a = dict(base)
    a.update(over)
    return getattr(L, name)(h, *[(v or None) if k in POINTERS else v for k, v in a.items()], None)


# (name of the argument, value) -> SEXTANS_ERR_INVALID, on both entry points where the argument exists
BAD = [("op", 0), ("op", 5), ("op", -1), ("N", 0), ("N", 4), ("N", 12), ("N", -8), ("N", 128 * 65535 + 8),
       ("ldb", 8), ("ldb", 18), ("lde", 12), ("lde", 17), ("B", 8), ("E", 52)]
BAD_FWD = [("ldc", 0), ("ldc", 22), ("C", 4)]
BAD_BWD = [("ldg", 15), ("ldg", 18), ("lddb", 8), ("lddb", 21), ("ldde", 12), ("ldde", 19), ("G", 84), ("dB", 100), ("dE", 120)]


def test_symbols_exported(sx):
    from sextans_amd import api
    api.lib()
    raw = C.CDLL(api.LIB_PATH)
    for name in (FWD_NAME, BWD_NAME):
        assert name in api._OPTIONAL_SYMBOLS and hasattr(raw, name), name
    assert (api.EDGE_MUL, api.EDGE_ADD, api.EDGE_ADD_RELU, api.EDGE_COPY) == (1, 2, 3, 4)


@pytest.mark.parametrize("fake", [False, True])
def test_argument_checks(sx, fake):
    from sextans_amd import api
    L = api.lib()
    h = (C.c_char * (1 << 20))()   # a handle without a matrix (zeroed engine state)
    hp = C.addressof(h) if fake else None
    # a NULL handle is INVALID whatever else is passed; aligned, valid arguments on a handle without a CSR matrix: STATE, before any
    # device is touched
    want = STATE if fake else INVALID
    big = 128 * 65535   # the largest N: 65535 tiles
    for op in (MUL, ADD, ADD_RELU, COPY):
        assert call(L, FWD_NAME, hp, FWD, op=op) == want, op
        assert call(L, BWD_NAME, hp, BWD, op=op, dB=0 if op == COPY else BWD["dB"]) == want, op
    assert call(L, FWD_NAME, hp, FWD, ldb=20, lde=24, ldc=28) == want          # any ld >= N that is a multiple of 4
    assert call(L, BWD_NAME, hp, BWD, ldb=20, lde=24, ldg=28, lddb=32, ldde=36) == want
    assert call(L, FWD_NAME, hp, FWD, N=264, ldb=264, lde=268, ldc=272) == want   # N has no upper limit but the tiles: more tiles
    assert call(L, BWD_NAME, hp, BWD, N=264, ldb=264, lde=268, ldg=264, lddb=272, ldde=264) == want
    assert call(L, FWD_NAME, hp, FWD, N=big, ldb=big, lde=big, ldc=big) == want
    assert call(L, FWD_NAME, hp, FWD, op=COPY, B=0) == want                   # COPY reads no B
    assert call(L, BWD_NAME, hp, BWD, op=ADD, B=0, E=0) == want               # ADD's gradients read neither B nor E
    assert call(L, BWD_NAME, hp, BWD, op=ADD, B=0, E=0, ldb=32, lde=20) == want
    assert call(L, BWD_NAME, hp, BWD, op=COPY, B=0, E=0, dB=0) == want
    for op in (MUL, ADD, ADD_RELU):
        assert call(L, BWD_NAME, hp, BWD, op=op, dB=0) == want                # either gradient alone
        assert call(L, BWD_NAME, hp, BWD, op=op, dE=0) == want
    assert call(L, BWD_NAME, hp, BWD, op=MUL, dB=0, E=0) == want              # MUL: dE reads B only, dB reads E only
    assert call(L, BWD_NAME, hp, BWD, op=MUL, dE=0, B=0) == want
    for op in (MUL, ADD, ADD_RELU, COPY):
        assert call(L, BWD_NAME, hp, BWD, op=op, dB=0, dE=0) == INVALID, op   # nothing to compute
    assert call(L, BWD_NAME, hp, BWD, op=COPY) == INVALID                     # COPY has no dB
    assert call(L, BWD_NAME, hp, BWD, op=COPY, dE=0) == INVALID
    for key, value in BAD:
        assert call(L, FWD_NAME, hp, FWD, **{key: value}) == INVALID, (key, value)
        assert call(L, BWD_NAME, hp, BWD, **{key: value}) == INVALID, (key, value)
    # a leading dimension is checked whether or not its pointer is NULL
    assert call(L, FWD_NAME, hp, FWD, op=COPY, B=0, ldb=8) == INVALID
    assert call(L, BWD_NAME, hp, BWD, op=ADD, B=0, E=0, lde=18) == INVALID
    for key, value in BAD_FWD:
        assert call(L, FWD_NAME, hp, FWD, **{key: value}) == INVALID, (key, value)
    for key, value in BAD_BWD:
        assert call(L, BWD_NAME, hp, BWD, **{key: value}) == INVALID, (key, value)


def test_python_and_torch_surfaces(sx):
    from sextans_amd import api, torch_op
    fwd = ["op", "N", "d_B", "ldb", "d_E", "lde", "d_C", "ldc", "stream"]
    bwd = ["op", "N", "d_B", "ldb", "d_E", "lde", "d_G", "ldg", "d_dB", "lddb", "d_dE", "ldde", "stream"]
    for name, params in (("spmm_edge_device_rm", fwd), ("spmm_edge_backward_device_rm", bwd)):
        sig = inspect.signature(getattr(api.Engine, name)).parameters
        assert list(sig)[1:] == params, name
        assert sig["stream"].default is None
    sig = inspect.signature(torch_op.spmm_edge).parameters
    assert list(sig) == ["A", "B", "E", "op", "reduce", "fast"]
    assert sig["op"].default == "mul" and sig["reduce"].default == "sum" and sig["fast"].default is False
    sig = inspect.signature(torch_op.from_edge_index).parameters
    assert list(sig) == ["edge_index", "num_dst", "num_src", "values"] and sig["values"].default is None
    assert "spmm_edge" in torch_op.__doc__ and "from_edge_index" in torch_op.__doc__
    with open(os.path.join(ROOT, "include", "sextans_amd.h")) as f:
        text = " ".join(f.read().split())
    for name, value in (("MUL", 1), ("ADD", 2), ("ADD_RELU", 3), ("COPY", 4)):
        assert "#define SEXTANS_EDGE_%s %d" % (name, value) in text
    assert ("int sextans_spmm_edge_device_rm(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const float *d_E, int64_t lde, "
            "float *d_C, int64_t ldc, void *stream);") in text
    assert ("int sextans_spmm_edge_backward_device_rm(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const float *d_E, "
            "int64_t lde, const float *d_G, int64_t ldg, float *d_dB, int64_t lddb, float *d_dE, int64_t ldde, void *stream);") in text
