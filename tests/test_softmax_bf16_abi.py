"""bf16 edge tensors for the two per-channel softmax families (sextans_vector_attention_device_rm_bf16,
sextans_vector_attention_backward_device_rm_bf16, sextans_spmm_edge_softagg_device_rm_bf16,
sextans_spmm_edge_softagg_backward_device_rm_bf16) without a GPU: the symbols exist; every refusal of the fp32 twins comes back from the
bf16 entry points, in the same order, on a NULL handle and on a zeroed one -- the argument checks of test_vector_attention_abi.py and
test_spmm_edge_softagg_abi.py are run again, as they stand, against the bf16 names (the workspace size serves both dtypes and keeps its
name); a bf16 leading dimension that is no multiple of 4 and a bf16 pointer that is 8-byte but not 16-byte aligned are refused; the
Python surfaces expose the entry points."""
import ctypes as C
import inspect
import os

import pytest

import test_spmm_edge_softagg_abi as soft_abi
import test_vector_attention_abi as vatt_abi
from util import ROOT

INVALID, STATE = vatt_abi.INVALID, vatt_abi.STATE

NAMES = {vatt_abi: ("sextans_vector_attention_device_rm_bf16", "sextans_vector_attention_backward_device_rm_bf16"),
         soft_abi: ("sextans_spmm_edge_softagg_device_rm_bf16", "sextans_spmm_edge_softagg_backward_device_rm_bf16")}


def test_symbols_exported(sx):
    from sextans_amd import api
    api.lib()
    raw = C.CDLL(api.LIB_PATH)
    for pair in NAMES.values():
        for name in pair:
            assert name in api._OPTIONAL_SYMBOLS and hasattr(raw, name), name


@pytest.mark.parametrize("fake", [False, True])
@pytest.mark.parametrize("family", ["vector_attention", "spmm_edge_softagg"])
def test_every_refusal_of_the_fp32_twin_in_its_order(sx, monkeypatch, family, fake):
    """bad mode / op, bad N, bad and optional leading dimensions, misalignment, nothing to compute, a gradient of an unread operand, dt
    without its workspace, COPY with dB, too many tiles, then the handle's state: the twin's own test, pointed at the bf16 names"""
    mod = vatt_abi if family == "vector_attention" else soft_abi
    monkeypatch.setattr(mod, "FWD_NAME", NAMES[mod][0])
    monkeypatch.setattr(mod, "BWD_NAME", NAMES[mod][1])
    mod.test_argument_checks(sx, fake)


def test_bf16_leading_dimensions_and_alignment_before_the_state(sx):
    """the bf16 tensors' own rules: a leading dimension counts ELEMENTS and is a multiple of 4 (18 and 22 are even: 4-byte multiples in
    bf16, refused all the same), a pointer is 16-byte aligned (8 more than an aligned address is refused).  Each is INVALID on a zeroed
    handle, on which a valid call is STATE: the argument errors come before the state."""
    from sextans_amd import api
    L = api.lib()
    h = (C.c_char * (1 << 20))()
    hp = C.addressof(h)
    f, b = NAMES[vatt_abi]
    F, B = vatt_abi.FWD, vatt_abi.BWD
    assert vatt_abi.call(L, f, hp, F) == STATE and vatt_abi.call(L, b, hp, B) == STATE
    for over in (dict(lds=18), dict(lds=22), dict(ldd=18), dict(ldd=30), dict(S=F["S"] + 8), dict(D=F["D"] + 8), dict(lds=12), dict(ldd=8)):
        assert vatt_abi.call(L, f, hp, F, **over) == INVALID, over
        assert vatt_abi.call(L, b, hp, B, **over) == INVALID, over
    for over in (dict(ldds=18), dict(ldds=22), dict(lddd=18), dict(lddd=26), dict(dS=B["dS"] + 8), dict(dD=B["dD"] + 8), dict(ldds=12)):
        assert vatt_abi.call(L, b, hp, B, **over) == INVALID, over
    for over in (dict(lds=20, ldd=24), dict(lds=32, ldd=16)):   # any multiple of 4 that is >= N
        assert vatt_abi.call(L, f, hp, F, **over) == STATE, over
        assert vatt_abi.call(L, b, hp, B, ldds=20, lddd=28, **over) == STATE, over
    f, b = NAMES[soft_abi]
    F, B = soft_abi.FWD, soft_abi.BWD
    assert soft_abi.call(L, f, hp, F) == STATE and soft_abi.call(L, b, hp, B) == STATE
    for over in (dict(lde=18), dict(lde=22), dict(lde=12), dict(E=F["E"] + 8)):
        assert soft_abi.call(L, f, hp, F, **over) == INVALID, over
        assert soft_abi.call(L, b, hp, B, **over) == INVALID, over
    for over in (dict(ldde=18), dict(ldde=22), dict(ldde=12), dict(dE=B["dE"] + 8)):
        assert soft_abi.call(L, b, hp, B, **over) == INVALID, over
    assert soft_abi.call(L, f, hp, F, lde=20) == STATE and soft_abi.call(L, b, hp, B, lde=20, ldde=28) == STATE
    # a required pointer that is NULL comes after the state
    assert vatt_abi.call(L, NAMES[vatt_abi][0], hp, vatt_abi.FWD, S=0) == STATE
    assert vatt_abi.call(L, NAMES[vatt_abi][1], hp, vatt_abi.BWD, D=0) == STATE
    assert soft_abi.call(L, NAMES[soft_abi][0], hp, soft_abi.FWD, E=0) == STATE
    assert soft_abi.call(L, NAMES[soft_abi][1], hp, soft_abi.BWD, E=0) == STATE


def test_python_and_torch_surfaces(sx):
    from sextans_amd import api, edge_softagg, vector_attention
    for twin in ("vector_attention_device_rm", "vector_attention_backward_device_rm", "spmm_edge_softagg_device_rm",
                 "spmm_edge_softagg_backward_device_rm"):
        a, b = (inspect.signature(getattr(api.Engine, name)).parameters for name in (twin, twin + "_bf16"))
        assert list(a) == list(b) and b["stream"].default is None, twin
        L = api.lib()
        assert getattr(L, "sextans_" + twin + "_bf16").argtypes == getattr(L, "sextans_" + twin).argtypes, twin
    # the torch ops take the bf16 route by themselves: their parameter lists stay, their docstrings name the entry points
    assert list(inspect.signature(vector_attention.vector_attention).parameters) == ["A", "S", "V", "D", "return_lse", "fast"]
    assert list(inspect.signature(edge_softagg.spmm_edge_softagg).parameters) == ["A", "B", "E", "op", "t", "eps", "return_lse", "fast"]
    assert "sextans_vector_attention_device_rm_bf16" in vector_attention.vector_attention.__doc__
    assert "sextans_spmm_edge_softagg_device_rm_bf16" in edge_softagg.spmm_edge_softagg.__doc__
    with open(os.path.join(ROOT, "include", "sextans_amd.h")) as f:
        text = " ".join(f.read().split())
    assert ("int sextans_vector_attention_device_rm_bf16(sextans_handle_t h, int msg, int N, const uint16_t *d_S, int64_t lds, "
            "const float *d_V, int64_t ldv, const uint16_t *d_D, int64_t ldd, float *d_C, int64_t ldc, float *d_lse, int64_t ldlse, "
            "void *stream);") in text
    assert ("int sextans_vector_attention_backward_device_rm_bf16(sextans_handle_t h, int msg, int N, const uint16_t *d_S, int64_t lds, "
            "const float *d_V, int64_t ldv, const uint16_t *d_D, int64_t ldd, const float *d_C, int64_t ldc, const float *d_lse, "
            "int64_t ldlse, const float *d_G, int64_t ldg, uint16_t *d_dS, int64_t ldds, float *d_dV, int64_t lddv, uint16_t *d_dD, "
            "int64_t lddd, void *stream);") in text
    assert ("int sextans_spmm_edge_softagg_device_rm_bf16(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, "
            "const uint16_t *d_E, int64_t lde, const float *d_t, float *d_C, int64_t ldc, float *d_lse, int64_t ldlse, void *stream);") in text
    assert ("int sextans_spmm_edge_softagg_backward_device_rm_bf16(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, "
            "const uint16_t *d_E, int64_t lde, const float *d_t, const float *d_C, int64_t ldc, const float *d_lse, int64_t ldlse, "
            "const float *d_G, int64_t ldg, float *d_dB, int64_t lddb, uint16_t *d_dE, int64_t ldde, float *d_dt, float *d_work, "
            "void *stream);") in text
