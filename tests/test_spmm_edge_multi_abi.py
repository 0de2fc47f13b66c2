"""Edge-feature multi-aggregation (sextans_spmm_edge_multi_device_rm, sextans_spmm_edge_multi_backward_device_rm): the symbols exist, bad
arguments and a handle without a matrix are refused with error codes before any device is touched (no GPU needed), and the Python
surfaces expose them.  The refusals that read the matrix (a required operand that is NULL with nnz > 0) are checked on an engine in
test_spmm_edge_multi_gpu.py."""
import ctypes as C
import inspect
import os

import pytest

from util import ROOT

OK = 0
INVALID = 9
STATE = 12
MUL, ADD, ADD_RELU, COPY = 1, 2, 3, 4

# addresses (0 = NULL) and leading dimensions; "out" / "g": False passes a NULL struct pointer
FWD = dict(op=MUL, N=16, B=16, ldb=16, E=32, lde=16, sum=48, sumsq=64, max=80, min=96, ld_sum=16, ld_sumsq=16, ld_max=16, ld_min=16,
           argmax=112, argmin=128, ld_arg=16, out=True)
BWD = dict(op=MUL, N=16, B=16, ldb=16, E=32, lde=16, gsum=48, gsumsq=64, gmax=80, gmin=96, ld_gsum=16, ld_gsumsq=16, ld_gmax=16, ld_gmin=16,
           argmax=112, argmin=128, ld_arg=16, g=True, dB=144, lddb=16, dE=160, ldde=16)


def forward(L, h, **over):
    from sextans_amd import api
    a = dict(FWD)
    a.update(over)
    o = api.MultiOut(a["sum"] or None, a["sumsq"] or None, a["max"] or None, a["min"] or None, a["ld_sum"], a["ld_sumsq"], a["ld_max"],
                     a["ld_min"], a["argmax"] or None, a["argmin"] or None, a["ld_arg"])
    return L.sextans_spmm_edge_multi_device_rm(h, a["op"], a["N"], a["B"] or None, a["ldb"], a["E"] or None, a["lde"],
                                               C.byref(o) if a["out"] else None, None)


def backward(L, h, **over):
    from sextans_amd import api
    a = dict(BWD)
    a.update(over)
    g = api.MultiGrad(a["gsum"] or None, a["gsumsq"] or None, a["gmax"] or None, a["gmin"] or None, a["ld_gsum"], a["ld_gsumsq"], a["ld_gmax"],
                      a["ld_gmin"], a["argmax"] or None, a["argmin"] or None, a["ld_arg"])
    return L.sextans_spmm_edge_multi_backward_device_rm(h, a["op"], a["N"], a["B"] or None, a["ldb"], a["E"] or None, a["lde"],
                                                        C.byref(g) if a["g"] else None, a["dB"] or None, a["lddb"], a["dE"] or None, a["ldde"],
                                                        None)


# (name of the argument, value) -> SEXTANS_ERR_INVALID, on both entry points
BAD = [("op", 0), ("op", 5), ("op", -1), ("N", 0), ("N", 4), ("N", 12), ("N", -8), ("ldb", 8), ("ldb", 18), ("lde", 12), ("lde", 17),
       ("ld_arg", 12), ("ld_arg", 17), ("B", 8), ("E", 20), ("argmax", 72), ("argmin", 100)]
BAD_FWD = [("out", False), ("ld_sum", 0), ("ld_sumsq", 22), ("ld_max", 8), ("ld_min", 17), ("sum", 4), ("sumsq", 72), ("max", 8), ("min", 100),
           (("sum", "sumsq", "max", "min", "argmax", "argmin"), 0),          # no output requested
           (("max", "min"), 0), (("max",), 0), (("min",), 0)]                # an arg without its value
BAD_BWD = [("g", False), ("ld_gsum", 15), ("ld_gsumsq", 18), ("ld_gmax", 8), ("ld_gmin", 21), ("lddb", 8), ("lddb", 21), ("ldde", 12),
           ("ldde", 18), ("gsum", 52), ("gsumsq", 8), ("gmax", 84), ("gmin", 100), ("dB", 148), ("dE", 168),
           (("gsum", "gsumsq", "gmax", "gmin"), 0),                          # no gradient given
           (("argmax",), 0), (("argmin",), 0),                               # the gradient of an extreme without its arg
           (("dB", "dE"), 0)]                                                # nothing to compute


def over(key, value):
    return {key: value} if isinstance(key, str) else {k: value for k in key}


def test_symbols_exported(sx):
    from sextans_amd import api
    api.lib()
    raw = C.CDLL(api.LIB_PATH)
    for name in ("sextans_spmm_edge_multi_device_rm", "sextans_spmm_edge_multi_backward_device_rm"):
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
        assert forward(L, hp, op=op) == want
        assert backward(L, hp, op=op, dB=0 if op == COPY else 144) == want
    assert forward(L, hp, ldb=20, lde=24, ld_sum=24, ld_sumsq=28, ld_max=32, ld_min=36, ld_arg=40) == want   # any ld >= N that is a multiple of 4
    assert backward(L, hp, ldb=20, lde=24, ld_gsum=24, ld_gsumsq=28, ld_gmax=32, ld_gmin=36, ld_arg=40, lddb=44, ldde=48) == want
    assert forward(L, hp, op=COPY, B=0) == want                                # COPY does not read B
    assert backward(L, hp, op=COPY, B=0, dB=0) == want
    assert forward(L, hp, argmax=0, argmin=0) == want                          # inference: no args
    assert forward(L, hp, max=0, min=0, argmax=0, argmin=0) == want            # one group alone
    assert forward(L, hp, sum=0, sumsq=0) == want
    assert forward(L, hp, sumsq=0, min=0, argmin=0) == want                    # a NULL output inside a group
    assert forward(L, hp, sum=0, ld_sum=0, argmax=0, argmin=0, ld_arg=0) == want   # the ld of a pointer that is not given is not read
    assert backward(L, hp, gmax=0, gmin=0, argmax=0, argmin=0, ld_arg=0, ld_gmax=0) == want
    assert backward(L, hp, gsum=0, gsumsq=0) == want
    assert backward(L, hp, dB=0) == want                                      # either gradient alone
    assert backward(L, hp, dE=0) == want
    assert forward(L, hp, N=264, ldb=264, lde=264, ld_sum=264, ld_sumsq=264, ld_max=264, ld_min=264, ld_arg=264) == want   # no upper limit on N
    assert backward(L, hp, N=264, ldb=264, lde=264, ld_gsum=264, ld_gsumsq=264, ld_gmax=264, ld_gmin=264, ld_arg=268, lddb=264, ldde=264) == want
    for key, value in BAD:
        assert forward(L, hp, **over(key, value)) == INVALID, (key, value)
        assert backward(L, hp, **over(key, value)) == INVALID, (key, value)
    for key, value in BAD_FWD:
        assert forward(L, hp, **over(key, value)) == INVALID, (key, value)
    for key, value in BAD_BWD:
        assert backward(L, hp, **over(key, value)) == INVALID, (key, value)
    assert backward(L, hp, op=COPY) == INVALID                                 # COPY has no dB
    assert backward(L, hp, op=COPY, B=0) == INVALID
    # more column tiles than the long-row kernel's grid holds (tiles of 64 floats here)
    big = 64 * 65535 + 8
    lds = dict(ldb=big, lde=big, ld_sum=big, ld_sumsq=big, ld_max=big, ld_min=big, ld_arg=big)
    assert forward(L, hp, N=big, **lds) == INVALID
    assert forward(L, hp, N=big - 8, **{k: big - 8 for k in lds}) == want
    lds = dict(ldb=big, lde=big, ld_gsum=big, ld_gsumsq=big, ld_gmax=big, ld_gmin=big, ld_arg=big, lddb=big, ldde=big)
    assert backward(L, hp, N=big, **lds) == INVALID
    assert backward(L, hp, N=big - 8, **{k: big - 8 for k in lds}) == want


def test_python_and_torch_surfaces(sx):
    from sextans_amd import api, torch_op
    fwd = ["op", "N", "d_B", "ldb", "d_E", "lde", "out", "stream"]
    bwd = ["op", "N", "d_B", "ldb", "d_E", "lde", "g", "d_dB", "lddb", "d_dE", "ldde", "stream"]
    for name, params in (("spmm_edge_multi_device_rm", fwd), ("spmm_edge_multi_backward_device_rm", bwd)):
        sig = inspect.signature(getattr(api.Engine, name)).parameters
        assert list(sig)[1:] == params, name
        assert sig["stream"].default is None
    sig = inspect.signature(torch_op.spmm_edge_multi).parameters
    assert list(sig) == ["A", "B", "E", "op", "aggr", "eps", "fast"]
    assert sig["op"].default == "mul" and sig["aggr"].default == ("mean", "max", "min", "std") and sig["eps"].default == 1e-5
    assert sig["fast"].default is False
    sig = inspect.signature(torch_op.spmm_edge_reduce).parameters
    assert list(sig) == ["A", "B", "E", "op", "reduce", "return_arg", "fast"]
    assert sig["op"].default == "mul" and sig["reduce"].default == "amax" and sig["return_arg"].default is False and sig["fast"].default is False
    assert list(inspect.signature(torch_op.spmm_edge).parameters) == ["A", "B", "E", "op", "reduce", "fast"]   # as it was
    assert "spmm_edge_multi" in torch_op.__doc__ and "spmm_edge_reduce" in torch_op.__doc__
    with open(os.path.join(ROOT, "include", "sextans_amd.h")) as f:
        text = " ".join(f.read().split())
    assert ("int sextans_spmm_edge_multi_device_rm(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const float *d_E, "
            "int64_t lde, const sextans_multi_out *out, void *stream);") in text
    assert ("int sextans_spmm_edge_multi_backward_device_rm(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, "
            "const float *d_E, int64_t lde, const sextans_multi_grad *g, float *d_dB, int64_t lddb, float *d_dE, int64_t ldde, "
            "void *stream);") in text
