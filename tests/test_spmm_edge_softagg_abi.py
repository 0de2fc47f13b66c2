"""Softmax aggregation of edge-feature messages (sextans_spmm_edge_softagg_device_rm, sextans_spmm_edge_softagg_workspace_floats,
sextans_spmm_edge_softagg_backward_device_rm): the symbols exist, bad arguments and a handle without a matrix are refused with error codes
before any device is touched, in the order the header states (no GPU needed), and the Python surfaces expose them."""
import ctypes as C
import inspect
import os

import pytest

from util import ROOT

OK = 0
INVALID = 9
STATE = 12

MUL, ADD, ADD_RELU, COPY = 1, 2, 3, 4

FWD = dict(op=MUL, N=16, B=32, ldb=16, E=16, lde=16, t=128, C=48, ldc=16, lse=64, ldlse=16)
BWD = dict(op=MUL, N=16, B=32, ldb=16, E=16, lde=16, t=128, C=48, ldc=16, lse=64, ldlse=16, G=80, ldg=16, dB=96, lddb=16, dE=112, ldde=16,
           dt=144, work=160)

POINTERS = ("B", "E", "t", "C", "lse", "G", "dB", "dE", "dt", "work")   # passed as addresses: 0 = NULL

FWD_NAME, WORK_NAME, BWD_NAME = ("sextans_spmm_edge_softagg_device_rm", "sextans_spmm_edge_softagg_workspace_floats",
                                 "sextans_spmm_edge_softagg_backward_device_rm")


def call(L, name, h, base, **over):
    a = dict(base)
    a.update(over)
    return getattr(L, name)(h, *[(v or None) if k in POINTERS else v for k, v in a.items()], None)


# (name of the argument, value) -> SEXTANS_ERR_INVALID, on both entry points
BAD = [("op", 0), ("op", 5), ("op", -1), ("N", 0), ("N", 4), ("N", 12), ("N", -8), ("ldb", 8), ("ldb", 18), ("lde", 12), ("lde", 17),
       ("ldc", 0), ("ldc", 22), ("B", 8), ("E", 20), ("t", 132), ("C", 4), ("lse", 72)]
BAD_FWD = [("ldlse", 12), ("ldlse", 17)]
BAD_BWD = [("ldlse", 12), ("ldlse", 17), ("ldg", 15), ("ldg", 18), ("lddb", 8), ("lddb", 21), ("ldde", 8), ("ldde", 22), ("G", 84),
           ("dB", 100), ("dE", 120), ("dt", 148), ("work", 164)]


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
    for op in (MUL, ADD, ADD_RELU, COPY):
        nodb = dict(dB=0) if op == COPY else {}
        assert call(L, FWD_NAME, hp, FWD, op=op) == want
        assert call(L, BWD_NAME, hp, BWD, op=op, **nodb) == want
        assert call(L, FWD_NAME, hp, FWD, op=op, ldb=20, lde=24, ldc=28, ldlse=32) == want     # any ld >= N that is a multiple of 4
        assert call(L, BWD_NAME, hp, BWD, op=op, ldb=20, lde=24, ldc=36, ldlse=24, ldg=28, lddb=32, ldde=20, **nodb) == want
        assert call(L, FWD_NAME, hp, FWD, op=op, t=0) == want                                  # t = 1
        assert call(L, BWD_NAME, hp, BWD, op=op, t=0, **nodb) == want
        assert call(L, FWD_NAME, hp, FWD, op=op, lse=0) == want                                # inference: no lse ...
        assert call(L, FWD_NAME, hp, FWD, op=op, lse=0, ldlse=0) == want                       # ... and then its ld is not looked at
        assert call(L, BWD_NAME, hp, BWD, op=op, dB=0, dt=0, work=0) == want                   # each gradient alone
        assert call(L, BWD_NAME, hp, BWD, op=op, dB=0, dE=0) == want
        assert call(L, BWD_NAME, hp, BWD, op=op, dB=0, dt=0) == want                           # a workspace that is not needed is allowed
        assert call(L, BWD_NAME, hp, BWD, op=op, dB=0, lddb=0, dE=0, ldde=3) == want           # the ld of an absent gradient is ignored
        assert call(L, FWD_NAME, hp, FWD, op=op, N=264, ldb=264, lde=264, ldc=264, ldlse=264) == want   # N has no upper limit: more tiles
        assert call(L, BWD_NAME, hp, BWD, op=op, N=264, ldb=264, lde=272, ldc=264, ldlse=268, ldg=264, lddb=264, ldde=264, **nodb) == want
        assert call(L, BWD_NAME, hp, BWD, op=op, dB=0, dE=0, dt=0) == INVALID                  # nothing to compute
        assert call(L, BWD_NAME, hp, BWD, op=op, dB=0, dE=0, dt=0, work=0) == INVALID
        assert call(L, BWD_NAME, hp, BWD, op=op, work=0) == INVALID                            # dt needs the workspace
        assert call(L, BWD_NAME, hp, BWD, op=op, dB=0, dE=0, work=0) == INVALID
    assert call(L, BWD_NAME, hp, BWD, dE=0, dt=0, work=0) == want                              # dB alone (not COPY)
    # COPY: B is optional, with its leading dimension; dB is refused -- before the handle's state is looked at
    assert call(L, FWD_NAME, hp, FWD, op=COPY, B=0, ldb=0) == want
    assert call(L, BWD_NAME, hp, BWD, op=COPY, B=0, ldb=0, dB=0) == want
    assert call(L, FWD_NAME, hp, FWD, op=COPY, ldb=8) == INVALID                               # (a B that is given counts)
    assert call(L, FWD_NAME, hp, FWD, op=MUL, B=0, ldb=0) == INVALID                           # (the others: ldb always)
    assert call(L, BWD_NAME, hp, BWD, op=COPY) == INVALID
    assert call(L, BWD_NAME, hp, BWD, op=COPY, dE=0, dt=0, work=0) == INVALID
    # a required pointer that is NULL comes after the state: STATE on the fake handle, not INVALID
    for key in ("B", "E", "C"):
        assert call(L, FWD_NAME, hp, FWD, **{key: 0}) == want, key
    for key in ("B", "E", "C", "lse", "G"):
        assert call(L, BWD_NAME, hp, BWD, **{key: 0}) == want, key
    for key, value in BAD:
        assert call(L, FWD_NAME, hp, FWD, **{key: value}) == INVALID, (key, value)
        assert call(L, BWD_NAME, hp, BWD, **{key: value}) == INVALID, (key, value)
    for key, value in BAD_FWD:
        assert call(L, FWD_NAME, hp, FWD, **{key: value}) == INVALID, (key, value)
    for key, value in BAD_BWD:
        assert call(L, BWD_NAME, hp, BWD, **{key: value}) == INVALID, (key, value)
    # the workspace size mirrors sextans_spmm_softagg_workspace_floats: the error code negated
    assert L.sextans_spmm_edge_softagg_workspace_floats(hp, 16) == -want
    assert L.sextans_spmm_edge_softagg_workspace_floats(hp, 264) == -want
    for n in (0, 4, 12, -8):
        assert L.sextans_spmm_edge_softagg_workspace_floats(hp, n) == -INVALID, n


def test_python_and_torch_surfaces(sx):
    from sextans_amd import api, edge_softagg, torch_op
    fwd = ["op", "N", "d_B", "ldb", "d_E", "lde", "d_t", "d_C", "ldc", "d_lse", "ldlse", "stream"]
    bwd = ["op", "N", "d_B", "ldb", "d_E", "lde", "d_t", "d_C", "ldc", "d_lse", "ldlse", "d_G", "ldg", "d_dB", "lddb", "d_dE", "ldde", "d_dt",
           "d_work", "stream"]
    for name, params in (("spmm_edge_softagg_device_rm", fwd), ("spmm_edge_softagg_backward_device_rm", bwd)):
        sig = inspect.signature(getattr(api.Engine, name)).parameters
        assert list(sig)[1:] == params, name
        assert sig["stream"].default is None
    assert list(inspect.signature(api.Engine.spmm_edge_softagg_workspace_floats).parameters)[1:] == ["N"]
    sig = inspect.signature(edge_softagg.spmm_edge_softagg).parameters
    assert list(sig) == ["A", "B", "E", "op", "t", "eps", "return_lse", "fast"]
    assert sig["op"].default == "mul" and sig["t"].default == 1.0 and sig["eps"].default == 0.0
    assert sig["return_lse"].default is False and sig["fast"].default is False
    assert edge_softagg.__all__ == ["spmm_edge_softagg"]
    assert not hasattr(torch_op, "spmm_edge_softagg") and "sextans_amd.edge_softagg" in torch_op.__doc__
    with open(os.path.join(ROOT, "include", "sextans_amd.h")) as f:
        text = " ".join(f.read().split())
    assert ("int sextans_spmm_edge_softagg_device_rm(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const float *d_E, "
            "int64_t lde, const float *d_t, float *d_C, int64_t ldc, float *d_lse, int64_t ldlse, void *stream);") in text
    assert "int64_t sextans_spmm_edge_softagg_workspace_floats(sextans_handle_t h, int N);" in text
    assert ("int sextans_spmm_edge_softagg_backward_device_rm(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, "
            "const float *d_E, int64_t lde, const float *d_t, const float *d_C, int64_t ldc, const float *d_lse, int64_t ldlse, "
            "const float *d_G, int64_t ldg, float *d_dB, int64_t lddb, float *d_dE, int64_t ldde, float *d_dt, float *d_work, "
            "void *stream);") in text
