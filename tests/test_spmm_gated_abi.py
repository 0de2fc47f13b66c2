"""Gated aggregation (sextans_spmm_gated_device_rm, sextans_spmm_gated_workspace_floats, sextans_spmm_gated_backward_device_rm): the
symbols exist, bad arguments and a handle without a matrix are refused with error codes before any device is touched (no GPU needed),
and the Python surfaces expose them."""
import ctypes as C
import inspect
import itertools
import math
import os

import pytest

from util import ROOT

OK = 0
INVALID = 9
STATE = 12
SUM, NORM = 1, 2

FWD_NAME, WORK_NAME, BWD_NAME = ("sextans_spmm_gated_device_rm", "sextans_spmm_gated_workspace_floats",
                                 "sextans_spmm_gated_backward_device_rm")

# addresses (0 = NULL) and leading dimensions of a valid call at N = 16; nothing is dereferenced before the handle's state is checked
IN = dict(xdst=16, xsrc=32, v=48, e=64, ld_xdst=16, ld_xsrc=16, ld_v=16, ld_e=16)
GRAD = dict(dxdst=208, dxsrc=224, dv=240, de=256, ld_dxdst=16, ld_dxsrc=16, ld_dv=16, ld_de=16)
FWD = dict(mode=SUM, eps=1e-6, N=16, C=80, ldc=16, den=96, ldden=16, z=112, ldz=16)
BWD = dict(mode=SUM, eps=1e-6, N=16, C=80, ldc=16, den=96, ldden=16, G=128, ldg=16, Gz=144, ldgz=16, work=160)
IN_PTRS, GRAD_PTRS = ("xdst", "xsrc", "v", "e"), ("dxdst", "dxsrc", "dv", "de")


def structs(over):
    from sextans_amd import api
    a, g = dict(IN), dict(GRAD)
    a.update({k: v for k, v in over.items() if k in a})
    g.update({k: v for k, v in over.items() if k in g})
    gin, out = api.GatedIn(), api.GatedGrad()
    for k, v in a.items():
        setattr(gin, k if k.startswith("ld_") else "d_" + k, (v or None) if k in IN_PTRS else v)
    for k, v in g.items():
        setattr(out, k if k.startswith("ld_") else "d_" + k, (v or None) if k in GRAD_PTRS else v)
    return gin, out


def fwd(L, h, null_in=False, **over):
    gin, _ = structs(over)
    a = dict(FWD)
    a.update({k: v for k, v in over.items() if k in a})
    return L.sextans_spmm_gated_device_rm(h, a["mode"], a["eps"], a["N"], None if null_in else C.byref(gin), a["C"] or None, a["ldc"],
                                          a["den"] or None, a["ldden"], a["z"] or None, a["ldz"], None)


def bwd(L, h, null_in=False, null_out=False, **over):
    gin, out = structs(over)
    a = dict(BWD)
    a.update({k: v for k, v in over.items() if k in a})
    return L.sextans_spmm_gated_backward_device_rm(h, a["mode"], a["eps"], a["N"], None if null_in else C.byref(gin), a["C"] or None, a["ldc"],
                                                   a["den"] or None, a["ldden"], a["G"] or None, a["ldg"], a["Gz"] or None, a["ldgz"],
                                                   None if null_out else C.byref(out), a["work"] or None, None)


BAD_N = [("N", 0), ("N", 4), ("N", 12), ("N", -8), ("N", 64 * 65535 + 8)]
# a leading dimension below N or no multiple of 4, a pointer that is not 16-byte aligned: on every pointer of the operand struct ...
BAD_IN = [("ld_xdst", 8), ("ld_xdst", 18), ("ld_xsrc", 12), ("ld_xsrc", 17), ("ld_v", 0), ("ld_v", 22), ("ld_e", 15), ("ld_e", 18),
          ("xdst", 20), ("xsrc", 36), ("v", 56), ("e", 68)]
BAD_FWD = [("ldc", 0), ("ldc", 22), ("ldden", 8), ("ldden", 17), ("ldz", 12), ("ldz", 18), ("C", 84), ("den", 100), ("z", 120)]
# ... and of the gradient struct, and the backward's own
BAD_GRAD = [("ld_dxdst", 8), ("ld_dxdst", 18), ("ld_dxsrc", 15), ("ld_dxsrc", 21), ("ld_dv", 0), ("ld_dv", 22), ("ld_de", 12), ("ld_de", 17),
            ("dxdst", 212), ("dxsrc", 228), ("dv", 248), ("de", 260)]
BAD_BWD = [("ldg", 15), ("ldg", 18), ("ldgz", 8), ("ldgz", 21), ("G", 132), ("Gz", 152), ("work", 164)]
BAD_BWD_NORM = [("ldc", 0), ("ldc", 22), ("ldden", 8), ("ldden", 17), ("C", 84), ("den", 100)]   # (SUM ignores C and den)


def test_symbols_exported(sx):
    from sextans_amd import api
    api.lib()
    raw = C.CDLL(api.LIB_PATH)
    for name in (FWD_NAME, WORK_NAME, BWD_NAME):
        assert name in api._OPTIONAL_SYMBOLS and hasattr(raw, name), name
    assert (api.GATE_SUM, api.GATE_NORM) == (SUM, NORM)


@pytest.mark.parametrize("mode", [SUM, NORM])
@pytest.mark.parametrize("fake", [False, True])
def test_argument_checks(sx, fake, mode):
    from sextans_amd import api
    L = api.lib()
    h = (C.c_char * (1 << 20))()   # a handle without a matrix (zeroed engine state)
    hp = C.addressof(h) if fake else None
    # a NULL handle is INVALID whatever else is passed; aligned, valid arguments on a handle without a CSR matrix: STATE, before any
    # device is touched
    want = STATE if fake else INVALID
    assert fwd(L, hp, mode=mode) == want
    assert bwd(L, hp, mode=mode) == want
    assert fwd(L, hp, mode=mode, e=0) == want and bwd(L, hp, mode=mode, e=0) == want      # no edge features
    assert fwd(L, hp, mode=mode, e=0, ld_e=0) == want                                      # (a leading dimension without its pointer)
    assert fwd(L, hp, mode=mode, den=0) == want and fwd(L, hp, mode=mode, z=0) == want     # optional outputs
    assert fwd(L, hp, mode=mode, e=0, den=0, z=0, ldden=0, ldz=0) == want
    assert bwd(L, hp, mode=mode, Gz=0) == want and bwd(L, hp, mode=mode, Gz=0, ldgz=0) == want
    assert bwd(L, hp, mode=mode, e=0, Gz=0) == want                                        # dE without E: the gradient of z
    for keep in itertools.product((False, True), repeat=4):                                # each gradient subset
        sub = {name: (GRAD[name] if k else 0) for name, k in zip(GRAD_PTRS, keep)}
        assert bwd(L, hp, mode=mode, **sub) == (want if any(keep) else INVALID), keep
    big = dict(N=264, ld_xdst=264, ld_xsrc=264, ld_v=264, ld_e=264)                         # N has no upper limit: more tiles
    assert fwd(L, hp, mode=mode, ldc=264, ldden=264, ldz=264, **big) == want
    assert bwd(L, hp, mode=mode, ldc=264, ldden=264, ldg=264, ldgz=268, ld_dxdst=264, ld_dxsrc=264, ld_dv=264, ld_de=272, **big) == want
    pad = dict(ld_xdst=20, ld_xsrc=24, ld_v=28, ld_e=32)                                    # any ld >= N that is a multiple of 4
    assert fwd(L, hp, mode=mode, ldc=36, ldden=20, ldz=24, **pad) == want
    assert bwd(L, hp, mode=mode, ldc=36, ldden=20, ldg=24, ldgz=28, ld_dxdst=32, ld_dxsrc=20, ld_dv=24, ld_de=28, **pad) == want
    if mode == SUM:                                                                        # SUM ignores eps, C and den
        for eps in (0.0, -1.0, math.nan, math.inf):
            assert fwd(L, hp, mode=mode, eps=eps) == want and bwd(L, hp, mode=mode, eps=eps) == want
        assert bwd(L, hp, mode=mode, C=0, den=0, work=0) == want
        for key, value in BAD_BWD_NORM:
            assert bwd(L, hp, mode=mode, **{key: value}) == want, (key, value)
    else:
        for eps in (0.0, -1e-6, math.nan, math.inf, -math.inf):
            assert fwd(L, hp, mode=mode, eps=eps) == INVALID, eps
            assert bwd(L, hp, mode=mode, eps=eps) == INVALID, eps
        for key, value in BAD_BWD_NORM:
            assert bwd(L, hp, mode=mode, **{key: value}) == INVALID, (key, value)
    for bad in (0, 3, -1):
        assert fwd(L, hp, mode=bad) == INVALID and bwd(L, hp, mode=bad) == INVALID
    assert fwd(L, hp, mode=mode, null_in=True) == INVALID
    assert bwd(L, hp, mode=mode, null_in=True) == INVALID and bwd(L, hp, mode=mode, null_out=True) == INVALID
    for key, value in BAD_N + BAD_IN:
        assert fwd(L, hp, mode=mode, **{key: value}) == INVALID, (key, value)
        assert bwd(L, hp, mode=mode, **{key: value}) == INVALID, (key, value)
    for key, value in BAD_FWD:
        assert fwd(L, hp, mode=mode, **{key: value}) == INVALID, (key, value)
    for key, value in BAD_GRAD + BAD_BWD:
        assert bwd(L, hp, mode=mode, **{key: value}) == INVALID, (key, value)
    # the workspace size mirrors sextans_spmm_softagg_workspace_floats: the error code negated
    assert L.sextans_spmm_gated_workspace_floats(hp, mode, 16) == -want
    assert L.sextans_spmm_gated_workspace_floats(hp, mode, 264) == -want
    for n in (0, 4, 12, -8):
        assert L.sextans_spmm_gated_workspace_floats(hp, mode, n) == -INVALID, n
    assert L.sextans_spmm_gated_workspace_floats(hp, 0, 16) == -INVALID and L.sextans_spmm_gated_workspace_floats(hp, 3, 16) == -INVALID


def test_python_and_torch_surfaces(sx):
    from sextans_amd import api, gated, torch_op
    fwd_p = ["mode", "eps", "N", "gin", "d_C", "ldc", "d_den", "ldden", "d_z", "ldz", "stream"]
    bwd_p = ["mode", "eps", "N", "gin", "d_C", "ldc", "d_den", "ldden", "d_G", "ldg", "d_Gz", "ldgz", "out", "d_work", "stream"]
    for name, params in (("spmm_gated_device_rm", fwd_p), ("spmm_gated_backward_device_rm", bwd_p)):
        sig = inspect.signature(getattr(api.Engine, name)).parameters
        assert list(sig)[1:] == params, name
        assert sig["stream"].default is None
    assert list(inspect.signature(api.Engine.spmm_gated_workspace_floats).parameters)[1:] == ["mode", "N"]
    assert [f[0] for f in api.GatedIn._fields_] == ["d_xdst", "d_xsrc", "d_v", "d_e", "ld_xdst", "ld_xsrc", "ld_v", "ld_e"]
    assert [f[0] for f in api.GatedGrad._fields_] == ["d_dxdst", "d_dxsrc", "d_dv", "d_de", "ld_dxdst", "ld_dxsrc", "ld_dv", "ld_de"]
    sig = inspect.signature(gated.spmm_gated).parameters
    assert list(sig) == ["A", "x_dst", "x_src", "V", "E", "normalize", "eps", "return_edge", "fast"]
    assert sig["E"].default is None and sig["normalize"].default is False and sig["eps"].default == 1e-6
    assert sig["return_edge"].default is False and sig["fast"].default is False
    assert gated.__all__ == ["spmm_gated"]
    assert not hasattr(torch_op, "spmm_gated") and "sextans_amd.gated" in torch_op.__doc__
    with open(os.path.join(ROOT, "include", "sextans_amd.h")) as f:
        text = " ".join(f.read().split())
    assert "#define SEXTANS_GATE_SUM 1" in text and "#define SEXTANS_GATE_NORM 2" in text
    assert ("typedef struct { const float *d_xdst, *d_xsrc, *d_v, *d_e; int64_t ld_xdst, ld_xsrc, ld_v, ld_e; } sextans_gated_in;") in text
    assert ("typedef struct { float *d_dxdst, *d_dxsrc, *d_dv, *d_de; int64_t ld_dxdst, ld_dxsrc, ld_dv, ld_de; } sextans_gated_grad;") in text
    assert ("int sextans_spmm_gated_device_rm(sextans_handle_t h, int mode, float eps, int N, const sextans_gated_in *in, float *d_C, "
            "int64_t ldc, float *d_den, int64_t ldden, float *d_z, int64_t ldz, void *stream);") in text
    assert "int64_t sextans_spmm_gated_workspace_floats(sextans_handle_t h, int mode, int N);" in text
    assert ("int sextans_spmm_gated_backward_device_rm(sextans_handle_t h, int mode, float eps, int N, const sextans_gated_in *in, "
            "const float *d_C, int64_t ldc, const float *d_den, int64_t ldden, const float *d_G, int64_t ldg, const float *d_Gz, "
            "int64_t ldgz, const sextans_gated_grad *out, float *d_work, void *stream);") in text
