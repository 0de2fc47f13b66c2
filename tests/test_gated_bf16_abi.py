"""bf16 edge tensors for the gated aggregation (sextans_spmm_gated_device_rm_bf16, sextans_spmm_gated_backward_device_rm_bf16) without a
GPU: the symbols exist; every refusal of the fp32 twins comes back from the bf16 entry points, in the same order, on a NULL handle and
on a zeroed one -- test_spmm_gated_abi.test_argument_checks is run again, as it stands, on a library whose two fp32 names answer with
the bf16 functions (the structs have the same layout; the workspace size serves both dtypes and keeps its name); a bf16 leading
dimension that is no multiple of 4 and a bf16 pointer that is 8-byte but not 16-byte aligned are refused before the handle's state; the
Python surfaces expose the entry points."""
import ctypes as C
import inspect
import os

import pytest

import test_spmm_gated_abi as twin
from util import ROOT

INVALID, STATE, SUM, NORM = twin.INVALID, twin.STATE, twin.SUM, twin.NORM
FWD_NAME, BWD_NAME = "sextans_spmm_gated_device_rm_bf16", "sextans_spmm_gated_backward_device_rm_bf16"


class Bf16Lib:
    """the library, with the two fp32 gated names answered by the bf16 entry points"""

    def __init__(self, L):
        self._L = L

    def __getattr__(self, name):
        return getattr(self._L, {twin.FWD_NAME: FWD_NAME, twin.BWD_NAME: BWD_NAME}.get(name, name))


def test_symbols_exported(sx):
    from sextans_amd import api
    api.lib()
    raw = C.CDLL(api.LIB_PATH)
    for name in (FWD_NAME, BWD_NAME):
        assert name in api._OPTIONAL_SYMBOLS and hasattr(raw, name), name


@pytest.mark.parametrize("mode", [SUM, NORM])
@pytest.mark.parametrize("fake", [False, True])
def test_every_refusal_of_the_fp32_twin_in_its_order(sx, monkeypatch, fake, mode):
    """bad mode, bad eps, bad N, NULL structs, bad and optional leading dimensions, misalignment, nothing to compute, too many tiles, then
    the handle's state: the twin's own test, answered by the bf16 entry points"""
    from sextans_amd import api
    proxy = Bf16Lib(api.lib())
    assert proxy.sextans_spmm_gated_device_rm is api.lib().sextans_spmm_gated_device_rm_bf16
    assert proxy.sextans_spmm_gated_backward_device_rm is api.lib().sextans_spmm_gated_backward_device_rm_bf16
    assert proxy.sextans_spmm_gated_workspace_floats is api.lib().sextans_spmm_gated_workspace_floats
    monkeypatch.setattr(api, "lib", lambda: proxy)
    twin.test_argument_checks(sx, fake, mode)


@pytest.mark.parametrize("mode", [SUM, NORM])
def test_bf16_leading_dimensions_and_alignment_before_the_state(sx, mode):
    """the bf16 tensors' own rules: a leading dimension counts ELEMENTS and is a multiple of 4 (18 and 22 are even: 4-byte multiples in
    bf16, refused all the same), a pointer is 16-byte aligned (8 more than an aligned address is refused).  Each is INVALID on a zeroed
    handle, on which a valid call is STATE: the argument errors come before the state."""
    from sextans_amd import api
    L = Bf16Lib(api.lib())
    h = (C.c_char * (1 << 20))()
    hp = C.addressof(h)
    assert twin.fwd(L, hp, mode=mode) == STATE and twin.bwd(L, hp, mode=mode) == STATE
    for over in (dict(ld_e=18), dict(ld_e=22), dict(ld_e=12), dict(e=twin.IN["e"] + 8)):
        assert twin.fwd(L, hp, mode=mode, **over) == INVALID, over
        assert twin.bwd(L, hp, mode=mode, **over) == INVALID, over
    for over in (dict(ldz=18), dict(ldz=22), dict(ldz=12), dict(z=twin.FWD["z"] + 8)):
        assert twin.fwd(L, hp, mode=mode, **over) == INVALID, over
    for over in (dict(ldgz=18), dict(ldgz=22), dict(ldgz=12), dict(Gz=twin.BWD["Gz"] + 8), dict(ld_de=18), dict(ld_de=22), dict(ld_de=12),
                 dict(de=twin.GRAD["de"] + 8)):
        assert twin.bwd(L, hp, mode=mode, **over) == INVALID, over
    # any multiple of 4 that is >= N; a leading dimension whose pointer is NULL does not count
    assert twin.fwd(L, hp, mode=mode, ld_e=20, ldz=28) == STATE
    assert twin.bwd(L, hp, mode=mode, ld_e=20, ldgz=24, ld_de=28) == STATE
    assert twin.fwd(L, hp, mode=mode, e=0, ld_e=18, z=0, ldz=22) == STATE
    assert twin.bwd(L, hp, mode=mode, e=0, ld_e=18, Gz=0, ldgz=22, de=0, ld_de=18) == STATE
    # z without E, and dE without E: allowed, as in the twin
    assert twin.fwd(L, hp, mode=mode, e=0) == STATE and twin.bwd(L, hp, mode=mode, e=0) == STATE
    # a required pointer that is NULL comes after the state
    assert twin.fwd(L, hp, mode=mode, xdst=0) == STATE and twin.bwd(L, hp, mode=mode, G=0) == STATE


def test_python_and_torch_surfaces(sx):
    from sextans_amd import api, gated, gated_bf16
    L = api.lib()
    for name in ("spmm_gated_device_rm", "spmm_gated_backward_device_rm"):
        a, b = (inspect.signature(getattr(api.Engine, n)).parameters for n in (name, name + "_bf16"))
        assert list(a) == list(b) and b["stream"].default is None, name
        assert getattr(L, "sextans_" + name + "_bf16").argtypes == getattr(L, "sextans_" + name).argtypes, name
    # spmm_gated takes the bf16 route by itself: its parameter list stays, its docstring names the entry point
    sig = inspect.signature(gated.spmm_gated).parameters
    assert list(sig) == ["A", "x_dst", "x_src", "V", "E", "normalize", "eps", "return_edge", "fast"]
    assert "sextans_spmm_gated_device_rm_bf16" in gated.spmm_gated.__doc__
    # the sibling with z in bf16: the same parameter list and defaults
    sig16 = inspect.signature(gated_bf16.spmm_gated_bf16).parameters
    assert list(sig16) == list(sig) and all(sig16[k].default == sig[k].default for k in sig)
    assert sig16["E"].default is None and sig16["normalize"].default is False and sig16["eps"].default == 1e-6
    assert sig16["return_edge"].default is False and sig16["fast"].default is False
    assert gated_bf16.__all__ == ["spmm_gated_bf16"]
    with open(os.path.join(ROOT, "include", "sextans_amd.h")) as f:
        text = " ".join(f.read().split())
    assert ("typedef struct { const float *d_xdst, *d_xsrc, *d_v; const uint16_t *d_e; int64_t ld_xdst, ld_xsrc, ld_v, ld_e; } "
            "sextans_gated_in_bf16;") in text
    assert ("typedef struct { float *d_dxdst, *d_dxsrc, *d_dv; uint16_t *d_de; int64_t ld_dxdst, ld_dxsrc, ld_dv, ld_de; } "
            "sextans_gated_grad_bf16;") in text
    assert ("int sextans_spmm_gated_device_rm_bf16(sextans_handle_t h, int mode, float eps, int N, const sextans_gated_in_bf16 *in, "
            "float *d_C, int64_t ldc, float *d_den, int64_t ldden, uint16_t *d_z, int64_t ldz, void *stream);") in text
    assert ("int sextans_spmm_gated_backward_device_rm_bf16(sextans_handle_t h, int mode, float eps, int N, const sextans_gated_in_bf16 *in, "
            "const float *d_C, int64_t ldc, const float *d_den, int64_t ldden, const float *d_G, int64_t ldg, const uint16_t *d_Gz, "
            "int64_t ldgz, const sextans_gated_grad_bf16 *out, float *d_work, void *stream);") in text
