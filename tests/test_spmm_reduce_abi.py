"""Max / min aggregation SpMM (sextans_spmm_reduce_device_rm, sextans_spmm_reduce_backward_device_rm): the symbols exist, bad arguments
and a handle without a matrix are refused with error codes before any device is touched (no GPU needed), and the Python surfaces expose
them."""
import ctypes as C
import inspect
import os

import pytest

from util import ROOT

OK = 0
INVALID = 9
STATE = 12

FWD = dict(op=1, N=16, val=16, B=32, ldb=16, C=48, ldc=16, arg=64, ldarg=16)
BWD = dict(N=16, val=16, B=32, ldb=16, arg=64, ldarg=16, G=80, ldg=16, dB=96, lddb=16, dval=112)

POINTERS = ("val", "B", "C", "arg", "G", "dB", "dval")   # passed as addresses: 0 = NULL


def call(L, name, h, base, **over):
    a = dict(base)
    a.update(over)
    return getattr(L, name)(h, *[(v or None) if k in POINTERS else v for k, v in a.items()], None)


# (name of the argument, value) -> SEXTANS_ERR_INVALID, on both entry points where the argument exists
BAD = [("N", 0), ("N", 4), ("N", 12), ("N", -8), ("ldb", 8), ("ldb", 18), ("ldarg", 12), ("ldarg", 17),
       ("val", 20), ("B", 8), ("arg", 72)]
BAD_FWD = [("op", 0), ("op", 3), ("op", -1), ("ldc", 0), ("ldc", 22), ("C", 4)]
BAD_BWD = [("ldg", 15), ("ldg", 18), ("lddb", 8), ("lddb", 21), ("G", 84), ("dB", 100), ("dval", 120)]


def test_symbols_exported(sx):
    from sextans_amd import api
    api.lib()
    raw = C.CDLL(api.LIB_PATH)
    for name in ("sextans_spmm_reduce_device_rm", "sextans_spmm_reduce_backward_device_rm"):
        assert name in api._OPTIONAL_SYMBOLS and hasattr(raw, name), name
    assert (api.REDUCE_MAX, api.REDUCE_MIN) == (1, 2)


@pytest.mark.parametrize("fake", [False, True])
def test_argument_checks(sx, fake):
    from sextans_amd import api
    L = api.lib()
    h = (C.c_char * (1 << 20))()   # a handle without a matrix (zeroed engine state)
    hp = C.addressof(h) if fake else None
    # a NULL handle is INVALID whatever else is passed; aligned, valid arguments on a handle without a CSR matrix: STATE, before any
    # device is touched
    want = STATE if fake else INVALID
    fwd, bwd = "sextans_spmm_reduce_device_rm", "sextans_spmm_reduce_backward_device_rm"
    assert call(L, fwd, hp, FWD) == want
    assert call(L, fwd, hp, FWD, op=2) == want
    assert call(L, bwd, hp, BWD) == want
    assert call(L, fwd, hp, FWD, ldb=20, ldc=24, ldarg=28) == want     # any ld >= N that is a multiple of 4
    assert call(L, bwd, hp, BWD, ldb=20, ldarg=24, ldg=28, lddb=32) == want
    assert call(L, fwd, hp, FWD, arg=0) == want                        # inference: no arg
    assert call(L, fwd, hp, FWD, val=0) == want                        # the engine's own values
    assert call(L, bwd, hp, BWD, val=0) == want
    assert call(L, bwd, hp, BWD, dB=0) == want                         # either gradient alone
    assert call(L, bwd, hp, BWD, dval=0, B=0) == want
    assert call(L, fwd, hp, FWD, N=264, ldb=264, ldc=264, ldarg=264) == want   # N has no upper limit: more tiles
    assert call(L, bwd, hp, BWD, N=264, ldb=264, ldarg=268, ldg=264, lddb=264) == want
    assert call(L, bwd, hp, BWD, dB=0, dval=0) == INVALID              # nothing to compute
    for key, value in BAD:
        assert call(L, fwd, hp, FWD, **{key: value}) == INVALID, (key, value)
        assert call(L, bwd, hp, BWD, **{key: value}) == INVALID, (key, value)
    for key, value in BAD_FWD:
        assert call(L, fwd, hp, FWD, **{key: value}) == INVALID, (key, value)
    for key, value in BAD_BWD:
        assert call(L, bwd, hp, BWD, **{key: value}) == INVALID, (key, value)


def test_python_and_torch_surfaces(sx):
    from sextans_amd import api, torch_op
    fwd = ["op", "N", "d_val", "d_B", "ldb", "d_C", "ldc", "d_arg", "ldarg", "stream"]
    bwd = ["N", "d_val", "d_B", "ldb", "d_arg", "ldarg", "d_G", "ldg", "d_dB", "lddb", "d_dval", "stream"]
    for name, params in (("spmm_reduce_device_rm", fwd), ("spmm_reduce_backward_device_rm", bwd)):
        sig = inspect.signature(getattr(api.Engine, name)).parameters
        assert list(sig)[1:] == params, name
        assert sig["stream"].default is None
    sig = inspect.signature(torch_op.spmm_reduce).parameters
    assert list(sig) == ["A", "B", "reduce", "return_arg", "fast"]
    assert sig["reduce"].default == "amax" and sig["return_arg"].default is False and sig["fast"].default is False
    assert "spmm_reduce" in torch_op.__doc__
    with open(os.path.join(ROOT, "include", "sextans_amd.h")) as f:
        text = " ".join(f.read().split())
    assert "#define SEXTANS_REDUCE_MAX 1" in text and "#define SEXTANS_REDUCE_MIN 2" in text
    assert ("int sextans_spmm_reduce_device_rm(sextans_handle_t h, int op, int N, const float *d_val, const float *d_B, int64_t ldb, "
            "float *d_C, int64_t ldc, int32_t *d_arg, int64_t ldarg, void *stream);") in text
    assert ("int sextans_spmm_reduce_backward_device_rm(sextans_handle_t h, int N, const float *d_val, const float *d_B, int64_t ldb, "
            "const int32_t *d_arg, int64_t ldarg, const float *d_G, int64_t ldg, float *d_dB, int64_t lddb, float *d_dval, "
            "void *stream);") in text
