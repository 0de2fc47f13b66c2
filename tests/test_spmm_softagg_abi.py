"""Softmax aggregation SpMM (sextans_spmm_softagg_device_rm, sextans_spmm_softagg_workspace_floats,
sextans_spmm_softagg_backward_device_rm): the symbols exist, bad arguments and a handle without a matrix are refused with error codes
before any device is touched (no GPU needed), and the Python surfaces expose them."""
import ctypes as C
import inspect
import os

import pytest

from test_spmm_reduce_abi import BAD as REDUCE_BAD
from util import ROOT

OK = 0
INVALID = 9
STATE = 12

FWD = dict(N=16, val=16, B=32, ldb=16, t=128, C=48, ldc=16, lse=64, ldlse=16)
BWD = dict(N=16, val=16, B=32, ldb=16, t=128, C=48, ldc=16, lse=64, ldlse=16, G=80, ldg=16, dB=96, lddb=16, dval=112, dt=144, work=160)

POINTERS = ("val", "B", "t", "C", "lse", "G", "dB", "dval", "dt", "work")   # passed as addresses: 0 = NULL

FWD_NAME, WORK_NAME, BWD_NAME = ("sextans_spmm_softagg_device_rm", "sextans_spmm_softagg_workspace_floats",
                                 "sextans_spmm_softagg_backward_device_rm")


def call(L, name, h, base, **over):
    a = dict(base)
    a.update(over)
    return getattr(L, name)(h, *[(v or None) if k in POINTERS else v for k, v in a.items()], None)


# the bad N, ld and alignment of the reduce family's list (its arg and ldarg: this family's lse and ldlse), on both entry points
BAD = [({"arg": "lse", "ldarg": "ldlse"}.get(k, k), v) for k, v in REDUCE_BAD]
BAD_BOTH = [("ldc", 0), ("ldc", 22), ("C", 4), ("t", 132)]
BAD_BWD = [("ldg", 15), ("ldg", 18), ("lddb", 8), ("lddb", 21), ("G", 84), ("dB", 100), ("dval", 120), ("dt", 148), ("work", 164)]


def test_symbols_exported(sx):
    from sextans_amd import api
    api.lib()
    raw = C.CDLL(api.LIB_PATH)
    for name in (FWD_NAME, WORK_NAME, BWD_NAME):
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
    assert ("N", 4) in BAD and ("ldlse", 17) in BAD and ("lse", 72) in BAD
    assert call(L, FWD_NAME, hp, FWD) == want
    assert call(L, BWD_NAME, hp, BWD) == want
    assert call(L, FWD_NAME, hp, FWD, ldb=20, ldc=24, ldlse=28) == want     # any ld >= N that is a multiple of 4
    assert call(L, BWD_NAME, hp, BWD, ldb=20, ldc=36, ldlse=24, ldg=28, lddb=32) == want
    assert call(L, FWD_NAME, hp, FWD, t=0) == want                          # t = 1
    assert call(L, BWD_NAME, hp, BWD, t=0) == want
    assert call(L, FWD_NAME, hp, FWD, lse=0) == want                        # inference: no lse
    assert call(L, FWD_NAME, hp, FWD, val=0) == want                        # the engine's own values
    assert call(L, BWD_NAME, hp, BWD, val=0) == want
    assert call(L, BWD_NAME, hp, BWD, dval=0, dt=0, work=0) == want         # each gradient alone
    assert call(L, BWD_NAME, hp, BWD, dB=0, dt=0, work=0) == want
    assert call(L, BWD_NAME, hp, BWD, dB=0, dval=0) == want
    assert call(L, BWD_NAME, hp, BWD, dt=0) == want                         # a workspace that is not needed is allowed
    assert call(L, FWD_NAME, hp, FWD, N=264, ldb=264, ldc=264, ldlse=264) == want   # N has no upper limit: more tiles
    assert call(L, BWD_NAME, hp, BWD, N=264, ldb=264, ldc=264, ldlse=268, ldg=264, lddb=264) == want
    assert call(L, BWD_NAME, hp, BWD, dB=0, dval=0, dt=0) == INVALID        # nothing to compute
    assert call(L, BWD_NAME, hp, BWD, dB=0, dval=0, dt=0, work=0) == INVALID
    assert call(L, BWD_NAME, hp, BWD, work=0) == INVALID                    # dt needs the workspace
    assert call(L, BWD_NAME, hp, BWD, dB=0, dval=0, work=0) == INVALID
    for key, value in BAD + BAD_BOTH:
        assert call(L, FWD_NAME, hp, FWD, **{key: value}) == INVALID, (key, value)
        assert call(L, BWD_NAME, hp, BWD, **{key: value}) == INVALID, (key, value)
    for key, value in BAD_BWD:
        assert call(L, BWD_NAME, hp, BWD, **{key: value}) == INVALID, (key, value)
    # the workspace size mirrors sextans_gatv2_workspace_floats: the error code negated
    assert L.sextans_spmm_softagg_workspace_floats(hp, 16) == -want
    assert L.sextans_spmm_softagg_workspace_floats(hp, 264) == -want
    for n in (0, 4, 12, -8):
        assert L.sextans_spmm_softagg_workspace_floats(hp, n) == -INVALID, n


def test_python_and_torch_surfaces(sx):
    from sextans_amd import api, torch_op
    fwd = ["N", "d_val", "d_B", "ldb", "d_t", "d_C", "ldc", "d_lse", "ldlse", "stream"]
    bwd = ["N", "d_val", "d_B", "ldb", "d_t", "d_C", "ldc", "d_lse", "ldlse", "d_G", "ldg", "d_dB", "lddb", "d_dval", "d_dt", "d_work", "stream"]
    for name, params in (("spmm_softagg_device_rm", fwd), ("spmm_softagg_backward_device_rm", bwd)):
        sig = inspect.signature(getattr(api.Engine, name)).parameters
        assert list(sig)[1:] == params, name
        assert sig["stream"].default is None
    assert list(inspect.signature(api.Engine.spmm_softagg_workspace_floats).parameters)[1:] == ["N"]
    sig = inspect.signature(torch_op.spmm_softagg).parameters
    assert list(sig) == ["A", "B", "t", "return_lse", "fast"]
    assert sig["t"].default == 1.0 and sig["return_lse"].default is False and sig["fast"].default is False
    assert "spmm_softagg" in torch_op.__doc__
    with open(os.path.join(ROOT, "include", "sextans_amd.h")) as f:
        text = " ".join(f.read().split())
    assert ("int sextans_spmm_softagg_device_rm(sextans_handle_t h, int N, const float *d_val, const float *d_B, int64_t ldb, "
            "const float *d_t, float *d_C, int64_t ldc, float *d_lse, int64_t ldlse, void *stream);") in text
    assert "int64_t sextans_spmm_softagg_workspace_floats(sextans_handle_t h, int N);" in text
    assert ("int sextans_spmm_softagg_backward_device_rm(sextans_handle_t h, int N, const float *d_val, const float *d_B, int64_t ldb, "
            "const float *d_t, const float *d_C, int64_t ldc, const float *d_lse, int64_t ldlse, const float *d_G, int64_t ldg, "
            "float *d_dB, int64_t lddb, float *d_dval, float *d_dt, float *d_work, void *stream);") in text
