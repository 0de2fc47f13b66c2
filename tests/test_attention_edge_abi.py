"""Edge features inside the fused attention (sextans_attention_edge_device, sextans_attention_edge_backward_device): the symbols exist,
bad arguments and a handle without a matrix are refused with error codes before any device is touched (no GPU needed), and the Python
surfaces expose them."""
import ctypes as C
import inspect
import os

import pytest

from util import ROOT

OK = 0
INVALID = 9
STATE = 12

# heads = 2, d = 16, dv = 24: rows of 32 and 48 floats
FWD = dict(heads=2, d=16, dv=24, scale=0.5, Q=64, ldq=32, K=128, ldk=32, V=192, ldv=48, Ek=256, ldek=32, Ev=320, ldev=48, bias=384,
           O=448, ldo=48, lse=512)
BWD = dict(heads=2, d=16, dv=24, scale=0.5, Q=64, ldq=32, K=128, ldk=32, V=192, ldv=48, Ek=256, ldek=32, Ev=320, ldev=48, bias=384,
           O=448, ldo=48, lse=512, G=576, ldg=48, delta=640, dQ=704, lddq=32, dK=768, lddk=32, dV=832, lddv=48, dEk=896, lddek=32,
           dEv=960, lddev=48, dbias=1024)
# d == dv: one dE buffer may take both gradients
SQUARE = dict(BWD, dv=16, ldv=32, ldev=32, ldo=32, ldg=32, lddv=32, lddev=32)

POINTERS = ("Q", "K", "V", "Ek", "Ev", "bias", "O", "lse", "G", "delta", "dQ", "dK", "dV", "dEk", "dEv", "dbias")   # addresses: 0 = NULL

FWD_NAME, BWD_NAME = "sextans_attention_edge_device", "sextans_attention_edge_backward_device"

# (argument, value) -> SEXTANS_ERR_INVALID on both entry points
BAD = [("heads", 0), ("heads", -1), ("d", 0), ("d", 4), ("d", 12), ("d", 136), ("dv", 0), ("dv", 20), ("dv", 136),
       ("ldq", 28), ("ldq", 34), ("ldk", 16), ("ldk", 33), ("ldv", 32), ("ldv", 50), ("ldek", 28), ("ldek", 34), ("ldev", 44), ("ldev", 49),
       ("ldo", 40), ("ldo", 49), ("Q", 68), ("K", 130), ("V", 200), ("Ek", 260), ("Ev", 328), ("bias", 388), ("O", 452), ("lse", 516)]
BAD_BWD = [("ldg", 40), ("ldg", 50), ("lddq", 16), ("lddq", 35), ("lddk", 28), ("lddk", 34), ("lddv", 24), ("lddv", 49),
           ("lddek", 28), ("lddek", 34), ("lddev", 44), ("lddev", 50), ("G", 580), ("delta", 644), ("dQ", 708), ("dK", 776), ("dV", 836),
           ("dEk", 900), ("dEv", 968), ("dbias", 1028)]


def call(L, name, h, base, drop=None, **over):
    a = dict(base)
    a.update(over)
    args = [(v or None) if k in POINTERS else v for k, v in a.items()]
    return getattr(L, name)(h, *args, C.byref(drop) if drop is not None else None, None)


def test_symbols_exported(sx):
    from sextans_amd import api
    api.lib()
    raw = C.CDLL(api.LIB_PATH)
    for name in (FWD_NAME, BWD_NAME):
        assert name in api._OPTIONAL_SYMBOLS and hasattr(raw, name), name


@pytest.mark.parametrize("fake", [False, True])
def test_argument_checks(sx, fake):
    from sextans_amd import api
    L, Drop = api.lib(), api.Dropout
    h = (C.c_char * (1 << 20))()   # a handle without a matrix (zeroed engine state)
    hp = C.addressof(h) if fake else None
    # a NULL handle is INVALID whatever else is passed; aligned, valid arguments on a handle without a CSR matrix: STATE, before any
    # device is touched
    want = STATE if fake else INVALID
    assert call(L, FWD_NAME, hp, FWD) == want
    assert call(L, BWD_NAME, hp, BWD) == want
    for absent in (dict(Ek=0), dict(Ev=0), dict(Ek=0, Ev=0)):   # key only / value only / neither: the plain entries
        assert call(L, FWD_NAME, hp, FWD, **absent) == want, absent
        grads = {"d" + k: 0 for k in absent}
        assert call(L, BWD_NAME, hp, BWD, **absent, **grads) == want, absent
    assert call(L, FWD_NAME, hp, FWD, bias=0) == want
    assert call(L, BWD_NAME, hp, BWD, bias=0, dbias=0) == want
    assert call(L, BWD_NAME, hp, BWD, dEk=0) == want              # either gradient alone, or neither
    assert call(L, BWD_NAME, hp, BWD, dEv=0) == want
    assert call(L, BWD_NAME, hp, BWD, dEk=0, dEv=0) == want
    assert call(L, BWD_NAME, hp, SQUARE) == want
    assert call(L, BWD_NAME, hp, SQUARE, dEv=SQUARE["dEk"]) == want   # d == dv: one shared gradient
    assert call(L, BWD_NAME, hp, SQUARE, dEv=SQUARE["dEk"], lddek=40, lddev=40) == want
    assert call(L, FWD_NAME, hp, FWD, ldq=36, ldk=40, ldv=52, ldek=44, ldev=56, ldo=60) == want   # any ld >= width that is a multiple of 4
    assert call(L, BWD_NAME, hp, BWD, ldg=52, lddq=36, lddk=40, lddv=56, lddek=44, lddev=60) == want
    assert call(L, FWD_NAME, hp, FWD, heads=1, d=128, dv=128, ldq=128, ldk=128, ldv=128, ldek=128, ldev=128, ldo=128) == want
    for drop in (Drop(0.0, 1, None), Drop(0.5, 7, None), Drop(0.25, 7, 4096)):
        assert call(L, FWD_NAME, hp, FWD, drop) == want
        assert call(L, BWD_NAME, hp, BWD, drop) == want
    for drop in (Drop(-0.1, 1, None), Drop(1.0, 1, None), Drop(float("nan"), 1, None), Drop(0.5, 1, 4100)):
        assert call(L, FWD_NAME, hp, FWD, drop) == INVALID
        assert call(L, BWD_NAME, hp, BWD, drop) == INVALID
        assert call(L, FWD_NAME, hp, FWD, drop, Ek=0, Ev=0) == INVALID
    for key, value in BAD:
        assert call(L, FWD_NAME, hp, FWD, **{key: value}) == INVALID, (key, value)
        assert call(L, BWD_NAME, hp, BWD, **{key: value}) == INVALID, (key, value)
    for key, value in BAD_BWD:
        assert call(L, BWD_NAME, hp, BWD, **{key: value}) == INVALID, (key, value)
    # a leading dimension is checked whether or not its pointer is NULL
    assert call(L, FWD_NAME, hp, FWD, Ek=0, ldek=28) == INVALID
    assert call(L, FWD_NAME, hp, FWD, Ev=0, ldev=50) == INVALID
    assert call(L, FWD_NAME, hp, FWD, Ek=0, Ev=0, ldek=0) == INVALID
    assert call(L, BWD_NAME, hp, BWD, Ek=0, dEk=0, ldek=30) == INVALID
    assert call(L, BWD_NAME, hp, BWD, dEk=0, lddek=28) == INVALID
    assert call(L, BWD_NAME, hp, BWD, Ek=0, Ev=0, dEk=0, dEv=0, lddev=46) == INVALID
    # a gradient pointer for an absent E
    assert call(L, BWD_NAME, hp, BWD, Ek=0) == INVALID
    assert call(L, BWD_NAME, hp, BWD, Ev=0) == INVALID
    assert call(L, BWD_NAME, hp, BWD, Ek=0, Ev=0) == INVALID
    assert call(L, BWD_NAME, hp, BWD, Ek=0, Ev=0, dEk=0) == INVALID
    # one buffer for both gradients: both E, d == dv and equal leading dimensions
    assert call(L, BWD_NAME, hp, BWD, dEv=BWD["dEk"]) == INVALID                          # d != dv
    assert call(L, BWD_NAME, hp, BWD, dEv=BWD["dEk"], lddek=48) == INVALID
    assert call(L, BWD_NAME, hp, SQUARE, dEv=SQUARE["dEk"], lddek=36) == INVALID          # lddek != lddev
    assert call(L, BWD_NAME, hp, SQUARE, dEv=SQUARE["dEk"], Ev=0) == INVALID              # an E is absent
    assert call(L, BWD_NAME, hp, SQUARE, dEv=SQUARE["dEk"], Ek=0) == INVALID


def test_python_and_torch_surfaces(sx):
    from sextans_amd import api, torch_op
    fwd = ["heads", "d", "dv", "scale", "d_Q", "ldq", "d_K", "ldk", "d_V", "ldv", "d_Ek", "ldek", "d_Ev", "ldev", "d_bias", "d_O", "ldo", "d_lse",
           "drop", "stream"]
    bwd = ["heads", "d", "dv", "scale", "d_Q", "ldq", "d_K", "ldk", "d_V", "ldv", "d_Ek", "ldek", "d_Ev", "ldev", "d_bias", "d_O", "ldo", "d_lse",
           "d_G", "ldg", "d_delta", "d_dQ", "lddq", "d_dK", "lddk", "d_dV", "lddv", "d_dEk", "lddek", "d_dEv", "lddev", "d_dbias", "drop", "stream"]
    for name, params in (("attention_edge_device", fwd), ("attention_edge_backward_device", bwd)):
        sig = inspect.signature(getattr(api.Engine, name)).parameters
        assert list(sig)[1:] == params, name
        assert sig["drop"].default is None and sig["stream"].default is None
    sig = inspect.signature(torch_op.sparse_attention_edge).parameters
    assert list(sig) == ["A", "Q", "K", "V", "edge_key", "edge_value", "scale", "bias", "dropout", "seed", "step", "fast"]
    assert sig["edge_key"].default is None and sig["edge_value"].default is None and sig["scale"].default is None
    assert sig["bias"].default is False and sig["dropout"].default == 0.0 and sig["seed"].default is None and sig["step"].default is None
    assert sig["fast"].default is False
    assert "sparse_attention_edge" in torch_op.__doc__
    # the existing functions keep their signatures
    assert list(inspect.signature(torch_op.sparse_attention).parameters) == ["A", "Q", "K", "V", "scale", "bias", "fast", "fused"]
    assert list(inspect.signature(torch_op.spmm_edge).parameters) == ["A", "B", "E", "op", "reduce", "fast"]
    with open(os.path.join(ROOT, "include", "sextans_amd.h")) as f:
        text = " ".join(f.read().split())
    assert ("int sextans_attention_edge_device(sextans_handle_t h, int heads, int d, int dv, float scale, const float *d_Q, int64_t ldq, "
            "const float *d_K, int64_t ldk, const float *d_V, int64_t ldv, const float *d_Ek, int64_t ldek, const float *d_Ev, int64_t ldev, "
            "const float *d_bias, float *d_O, int64_t ldo, float *d_lse, const sextans_dropout *drop, void *stream);") in text
    assert ("int sextans_attention_edge_backward_device(sextans_handle_t h, int heads, int d, int dv, float scale, const float *d_Q, int64_t ldq, "
            "const float *d_K, int64_t ldk, const float *d_V, int64_t ldv, const float *d_Ek, int64_t ldek, const float *d_Ev, int64_t ldev, "
            "const float *d_bias, const float *d_O, int64_t ldo, const float *d_lse, const float *d_G, int64_t ldg, float *d_delta, "
            "float *d_dQ, int64_t lddq, float *d_dK, int64_t lddk, float *d_dV, int64_t lddv, float *d_dEk, int64_t lddek, float *d_dEv, "
            "int64_t lddev, float *d_dbias, const sextans_dropout *drop, void *stream);") in text
