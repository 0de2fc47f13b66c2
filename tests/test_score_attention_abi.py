"""Attention from caller-supplied per-head scores (sextans_score_attention_device, sextans_score_attention_backward_device): the symbols
exist, bad arguments and a handle without a matrix are refused with error codes, in the documented order, before any device is touched
(no GPU needed), and the Python surfaces expose them."""
import ctypes as C
import inspect
import os

import pytest

from util import ROOT

OK = 0
INVALID = 9
STATE = 12
SOFTMAX, WEIGHT = 1, 2

FWD = dict(mode=SOFTMAX, heads=2, dv=16, S=16, lds=2, V=48, ldv=32, O=64, ldo=32, lse=80)
BWD = dict(mode=SOFTMAX, heads=2, dv=16, S=16, lds=2, V=48, ldv=32, O=64, ldo=32, lse=80, G=96, ldg=32, dS=112, ldds=2, dV=128, lddv=32)
POINTERS = ("S", "V", "O", "lse", "G", "dS", "dV")   # passed as addresses: 0 = NULL

# (name of the argument, value) -> SEXTANS_ERR_INVALID, on both entry points where the argument exists
BAD = [("mode", 0), ("mode", 3), ("heads", 0), ("heads", -1), ("dv", 0), ("dv", 12), ("dv", 136),
       ("lds", 1), ("ldv", 31), ("ldv", 16), ("ldv", 38), ("ldo", 0), ("ldo", 35),
       ("S", 20), ("V", 4), ("O", 72), ("lse", 84)]
BAD_BWD = [("ldg", 24), ("ldg", 37), ("ldds", 1), ("lddv", 8), ("lddv", 34), ("G", 100), ("dS", 116), ("dV", 132)]


def dropout(api, p):
    return C.byref(api.Dropout(p, 5, None))


def call(L, name, h, base, drop=None, **over):
    a = dict(base)
    a.update(over)
    return getattr(L, name)(h, *[(v or None) if k in POINTERS else v for k, v in a.items()], drop, None)


def test_symbols_exported(sx):
    from sextans_amd import api
    api.lib()
    raw = C.CDLL(api.LIB_PATH)
    for name in ("sextans_score_attention_device", "sextans_score_attention_backward_device"):
        assert name in api._OPTIONAL_SYMBOLS and hasattr(raw, name), name
    assert (api.SCORE_SOFTMAX, api.SCORE_WEIGHT) == (SOFTMAX, WEIGHT)


@pytest.mark.parametrize("fake", [False, True])
def test_argument_checks(sx, fake):
    from sextans_amd import api
    L = api.lib()
    h = (C.c_char * (1 << 20))()   # a handle without a matrix (zeroed engine state)
    hp = C.addressof(h) if fake else None
    # a NULL handle is INVALID whatever else is passed; aligned, valid arguments on a handle without a CSR matrix: STATE, before any
    # device is touched
    want = STATE if fake else INVALID
    fwd, bwd = "sextans_score_attention_device", "sextans_score_attention_backward_device"
    for mode in (SOFTMAX, WEIGHT):
        assert call(L, fwd, hp, FWD, mode=mode) == want
        assert call(L, bwd, hp, BWD, mode=mode) == want
        assert call(L, fwd, hp, FWD, mode=mode, lds=3) == want            # any lds >= heads: S is read one float at a time
        assert call(L, bwd, hp, BWD, mode=mode, lds=7, ldds=5) == want
        assert call(L, fwd, hp, FWD, mode=mode, heads=1, dv=128, lds=1, ldv=128, ldo=132) == want
        assert call(L, bwd, hp, BWD, mode=mode, heads=1, dv=8, ldv=8, ldo=8, ldg=12, lddv=8) == want
        assert call(L, bwd, hp, BWD, mode=mode, dS=0) == want and call(L, bwd, hp, BWD, mode=mode, dV=0) == want
        assert call(L, fwd, hp, FWD, dropout(api, 0.0), mode=mode) == want   # p == 0 is no dropout: fine in both modes
        assert call(L, bwd, hp, BWD, dropout(api, 0.0), mode=mode) == want
    assert call(L, fwd, hp, FWD, dropout(api, 0.5)) == want
    assert call(L, bwd, hp, BWD, dropout(api, 0.5)) == want
    assert call(L, fwd, hp, FWD, mode=WEIGHT, lse=0) == want              # WEIGHT touches neither lse nor (backward) O
    assert call(L, bwd, hp, BWD, mode=WEIGHT, O=0, lse=0, ldo=0) == want
    for key, value in BAD:
        assert call(L, fwd, hp, FWD, **{key: value}) == INVALID, (key, value)
        assert call(L, bwd, hp, BWD, **{key: value}) == INVALID, (key, value)
    for key, value in BAD_BWD:
        assert call(L, bwd, hp, BWD, **{key: value}) == INVALID, (key, value)
    for name, base in ((fwd, FWD), (bwd, BWD)):
        assert call(L, name, hp, base, dropout(api, 0.5), mode=WEIGHT) == INVALID    # the caller holds the weights and can drop them
        assert call(L, name, hp, base, dropout(api, 1.0)) == INVALID
        assert call(L, name, hp, base, dropout(api, -0.1)) == INVALID
    if fake:
        # the documented order: dimensions, dropout, leading dimensions and alignment come before the matrix state
        assert call(L, bwd, hp, BWD, dS=0, dV=0) == STATE                 # (NULL operands are looked at after it)


def test_python_and_torch_surfaces(sx):
    from sextans_amd import api, torch_op
    fwd = ["mode", "heads", "dv", "d_S", "lds", "d_V", "ldv", "d_O", "ldo", "d_lse", "drop", "stream"]
    bwd = ["mode", "heads", "dv", "d_S", "lds", "d_V", "ldv", "d_O", "ldo", "d_lse", "d_G", "ldg", "d_dS", "ldds", "d_dV", "lddv", "drop", "stream"]
    for name, params in (("score_attention_device", fwd), ("score_attention_backward_device", bwd)):
        sig = inspect.signature(getattr(api.Engine, name)).parameters
        assert list(sig)[1:] == params, name
        assert sig["stream"].default is None and list(sig)[-1] == "stream"
    sig = inspect.signature(torch_op.score_attention).parameters
    assert list(sig) == ["A", "S", "V", "normalize", "dropout", "seed", "step", "return_weights", "fast"]
    assert sig["normalize"].default == "softmax" and sig["dropout"].default == 0.0 and sig["seed"].default is None
    assert sig["step"].default is None and sig["return_weights"].default is False and sig["fast"].default is False
    assert list(inspect.signature(torch_op.entry_rows).parameters) == ["A"]
    assert "score_attention(" in torch_op.__doc__ and "entry_rows(" in torch_op.__doc__
    with open(os.path.join(ROOT, "include", "sextans_amd.h")) as f:
        text = " ".join(f.read().split())
    assert "#define SEXTANS_SCORE_SOFTMAX 1" in text and "#define SEXTANS_SCORE_WEIGHT 2" in text
    assert ("int sextans_score_attention_device(sextans_handle_t h, int mode, int heads, int dv, const float *d_S, int64_t lds, "
            "const float *d_V, int64_t ldv, float *d_O, int64_t ldo, float *d_lse, const sextans_dropout *drop, void *stream);") in text
    assert ("int sextans_score_attention_backward_device(sextans_handle_t h, int mode, int heads, int dv, const float *d_S, int64_t lds, "
            "const float *d_V, int64_t ldv, const float *d_O, int64_t ldo, const float *d_lse, const float *d_G, int64_t ldg, "
            "float *d_dS, int64_t ldds, float *d_dV, int64_t lddv, const sextans_dropout *drop, void *stream);") in text
