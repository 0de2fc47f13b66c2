"""Channel-wise attention from per-channel scores (sextans_vector_attention_device_rm, sextans_vector_attention_backward_device_rm): the
symbols exist, bad arguments and a handle without a matrix are refused with error codes before any device is touched, in the order the
header states (no GPU needed), and the Python surfaces expose them."""
import ctypes as C
import inspect
import os

import pytest

from util import ROOT

OK = 0
INVALID = 9
STATE = 12

NODE, ADD, EDGE = 1, 2, 3

FWD = dict(msg=ADD, N=16, S=16, lds=16, V=32, ldv=16, D=48, ldd=16, C=64, ldc=16, lse=80, ldlse=16)
BWD = dict(msg=ADD, N=16, S=16, lds=16, V=32, ldv=16, D=48, ldd=16, C=64, ldc=16, lse=80, ldlse=16, G=96, ldg=16, dS=112, ldds=16, dV=128,
           lddv=16, dD=144, lddd=16)

POINTERS = ("S", "V", "D", "C", "lse", "G", "dS", "dV", "dD")   # passed as addresses: 0 = NULL

FWD_NAME, BWD_NAME = "sextans_vector_attention_device_rm", "sextans_vector_attention_backward_device_rm"

# the gradients a mode has no operand for must not be asked for
NOT_OF = {NODE: dict(dD=0), ADD: {}, EDGE: dict(dV=0)}


def call(L, name, h, base, **over):
    a = dict(base)
    a.update(over)
    return getattr(L, name)(h, *[(v or None) if k in POINTERS else v for k, v in a.items()], None)


# (name of the argument, value) -> SEXTANS_ERR_INVALID, on both entry points, in ADD mode (which reads every operand)
BAD = [("msg", 0), ("msg", 4), ("msg", -1), ("N", 0), ("N", 4), ("N", 12), ("N", -8), ("lds", 8), ("lds", 18), ("ldv", 12), ("ldv", 17),
       ("ldd", 8), ("ldd", 21), ("ldc", 0), ("ldc", 22), ("S", 8), ("V", 36), ("D", 52), ("C", 68), ("lse", 88)]
BAD_FWD = [("ldlse", 12), ("ldlse", 17)]
BAD_BWD = [("ldlse", 12), ("ldlse", 17), ("ldg", 15), ("ldg", 18), ("ldds", 8), ("ldds", 21), ("lddv", 8), ("lddv", 22), ("lddd", 12),
           ("lddd", 18), ("G", 100), ("dS", 116), ("dV", 136), ("dD", 148)]


def test_symbols_exported(sx):
    from sextans_amd import api
    api.lib()
    raw = C.CDLL(api.LIB_PATH)
    for name in (FWD_NAME, BWD_NAME):
        assert name in api._OPTIONAL_SYMBOLS and hasattr(raw, name), name
    assert (api.VATT_NODE, api.VATT_ADD, api.VATT_EDGE) == (NODE, ADD, EDGE)


@pytest.mark.parametrize("fake", [False, True])
def test_argument_checks(sx, fake):
    from sextans_amd import api
    L = api.lib()
    h = (C.c_char * (1 << 20))()   # a handle without a matrix (zeroed engine state)
    hp = C.addressof(h) if fake else None
    # a NULL handle is INVALID whatever else is passed; aligned, valid arguments on a handle without a CSR matrix: STATE, before any
    # device is touched
    want = STATE if fake else INVALID
    for msg in (NODE, ADD, EDGE):
        no = NOT_OF[msg]
        assert call(L, FWD_NAME, hp, FWD, msg=msg) == want
        assert call(L, BWD_NAME, hp, BWD, msg=msg, **no) == want
        assert call(L, FWD_NAME, hp, FWD, msg=msg, lds=20, ldv=24, ldd=32, ldc=28, ldlse=32) == want   # any ld >= N that is a multiple of 4
        assert call(L, BWD_NAME, hp, BWD, msg=msg, lds=20, ldv=24, ldd=20, ldc=36, ldlse=24, ldg=28, ldds=32, lddv=20, lddd=24, **no) == want
        assert call(L, FWD_NAME, hp, FWD, msg=msg, lse=0) == want                                # inference: no lse ...
        assert call(L, FWD_NAME, hp, FWD, msg=msg, lse=0, ldlse=0) == want                       # ... and then its ld is not looked at
        assert call(L, BWD_NAME, hp, BWD, msg=msg, dV=0, dD=0) == want                           # dS alone
        assert call(L, BWD_NAME, hp, BWD, msg=msg, dV=0, lddv=0, dD=0, lddd=3) == want           # the ld of an absent gradient is ignored
        assert call(L, FWD_NAME, hp, FWD, msg=msg, N=264, lds=264, ldv=264, ldd=264, ldc=264, ldlse=264) == want   # N has no upper limit
        assert call(L, BWD_NAME, hp, BWD, msg=msg, N=264, lds=264, ldv=272, ldd=264, ldc=264, ldlse=268, ldg=264, ldds=264, lddv=264,
                    lddd=264, **no) == want
        assert call(L, BWD_NAME, hp, BWD, msg=msg, dS=0, dV=0, dD=0) == INVALID                  # nothing to compute
    # each gradient alone where the mode has it
    assert call(L, BWD_NAME, hp, BWD, msg=NODE, dS=0, dD=0) == want
    assert call(L, BWD_NAME, hp, BWD, msg=ADD, dS=0, dD=0) == want
    assert call(L, BWD_NAME, hp, BWD, msg=ADD, dS=0, dV=0) == want
    assert call(L, BWD_NAME, hp, BWD, msg=EDGE, dS=0, dV=0) == want
    # an operand the mode does not read is ignored: absent, misaligned or with any leading dimension
    for name in (FWD_NAME, BWD_NAME):
        base = FWD if name == FWD_NAME else BWD
        assert call(L, name, hp, base, msg=NODE, D=0, ldd=0, **(NOT_OF[NODE] if base is BWD else {})) == want
        assert call(L, name, hp, base, msg=NODE, D=52, ldd=3, **(NOT_OF[NODE] if base is BWD else {})) == want
        assert call(L, name, hp, base, msg=EDGE, V=0, ldv=0, **(NOT_OF[EDGE] if base is BWD else {})) == want
        assert call(L, name, hp, base, msg=EDGE, V=36, ldv=5, **(NOT_OF[EDGE] if base is BWD else {})) == want
        assert call(L, name, hp, base, msg=NODE, ldv=8, **(NOT_OF[NODE] if base is BWD else {})) == INVALID   # (one it reads counts)
        assert call(L, name, hp, base, msg=EDGE, ldd=8, **(NOT_OF[EDGE] if base is BWD else {})) == INVALID
    # a gradient of an operand the mode does not read is refused -- before the handle's state is looked at
    assert call(L, BWD_NAME, hp, BWD, msg=EDGE) == INVALID
    assert call(L, BWD_NAME, hp, BWD, msg=EDGE, dS=0, dD=0) == INVALID
    assert call(L, BWD_NAME, hp, BWD, msg=NODE) == INVALID
    assert call(L, BWD_NAME, hp, BWD, msg=NODE, dS=0, dV=0) == INVALID
    # a required pointer that is NULL comes after the state: STATE on the fake handle, not INVALID
    for key in ("S", "V", "D", "C"):
        assert call(L, FWD_NAME, hp, FWD, **{key: 0}) == want, key
    for key in ("S", "V", "D", "C", "lse", "G"):
        assert call(L, BWD_NAME, hp, BWD, **{key: 0}) == want, key
    for key, value in BAD:
        assert call(L, FWD_NAME, hp, FWD, **{key: value}) == INVALID, (key, value)
        assert call(L, BWD_NAME, hp, BWD, **{key: value}) == INVALID, (key, value)
    for key, value in BAD_FWD:
        assert call(L, FWD_NAME, hp, FWD, **{key: value}) == INVALID, (key, value)
    for key, value in BAD_BWD:
        assert call(L, BWD_NAME, hp, BWD, **{key: value}) == INVALID, (key, value)
    # more column tiles than the long-row kernel's grid has (65535 of 64 floats)
    big = 65536 * 64
    assert call(L, FWD_NAME, hp, FWD, N=big, lds=big, ldv=big, ldd=big, ldc=big, ldlse=big) == INVALID
    assert call(L, BWD_NAME, hp, BWD, N=big, lds=big, ldv=big, ldd=big, ldc=big, ldlse=big, ldg=big, ldds=big, lddv=big, lddd=big) == INVALID


def test_python_and_torch_surfaces(sx):
    from sextans_amd import api, torch_op, vector_attention
    fwd = ["msg", "N", "d_S", "lds", "d_V", "ldv", "d_D", "ldd", "d_C", "ldc", "d_lse", "ldlse", "stream"]
    bwd = ["msg", "N", "d_S", "lds", "d_V", "ldv", "d_D", "ldd", "d_C", "ldc", "d_lse", "ldlse", "d_G", "ldg", "d_dS", "ldds", "d_dV", "lddv",
           "d_dD", "lddd", "stream"]
    for name, params in (("vector_attention_device_rm", fwd), ("vector_attention_backward_device_rm", bwd)):
        sig = inspect.signature(getattr(api.Engine, name)).parameters
        assert list(sig)[1:] == params, name
        assert sig["stream"].default is None
    sig = inspect.signature(vector_attention.vector_attention).parameters
    assert list(sig) == ["A", "S", "V", "D", "return_lse", "fast"]
    assert sig["V"].default is None and sig["D"].default is None
    assert sig["return_lse"].default is False and sig["fast"].default is False
    assert vector_attention.__all__ == ["vector_attention"]
    assert not hasattr(torch_op, "vector_attention") and "sextans_amd.vector_attention" in torch_op.__doc__
    with open(os.path.join(ROOT, "include", "sextans_amd.h")) as f:
        text = " ".join(f.read().split())
    assert ("int sextans_vector_attention_device_rm(sextans_handle_t h, int msg, int N, const float *d_S, int64_t lds, const float *d_V, "
            "int64_t ldv, const float *d_D, int64_t ldd, float *d_C, int64_t ldc, float *d_lse, int64_t ldlse, void *stream);") in text
    assert ("int sextans_vector_attention_backward_device_rm(sextans_handle_t h, int msg, int N, const float *d_S, int64_t lds, "
            "const float *d_V, int64_t ldv, const float *d_D, int64_t ldd, const float *d_C, int64_t ldc, const float *d_lse, "
            "int64_t ldlse, const float *d_G, int64_t ldg, float *d_dS, int64_t ldds, float *d_dV, int64_t lddv, float *d_dD, "
            "int64_t lddd, void *stream);") in text
    for name in ("SEXTANS_VATT_NODE 1", "SEXTANS_VATT_ADD 2", "SEXTANS_VATT_EDGE 3"):
        assert "#define " + name in text
