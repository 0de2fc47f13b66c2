"""bf16 edge tensors for the edge-output ops and the edge-feature SpMM (sextans_edge_op_device_rm_bf16, sextans_edge_op_backward_device_rm_bf16,
sextans_spmm_edge_device_rm_bf16, sextans_spmm_edge_backward_device_rm_bf16) without a GPU: the symbols exist; every refusal of the fp32
twins comes back from the bf16 entry points, in the same order, on a NULL handle and on a zeroed one -- the argument checks of
test_edge_op_abi.py and test_spmm_edge_abi.py are run again, as they stand, against the bf16 names; the Python surfaces expose the
route; and the host rounding the GPU tests rely on (to_bf16: torch's CPU float32 -> bfloat16) is the rule of the header on a fixed
list of values: ties both ways, the largest finite fp32, denormals, +-0, +-inf, NaN."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import test_edge_op_abi as op_abi
import test_spmm_edge_abi as edge_abi
from util import ROOT

INVALID, STATE = op_abi.INVALID, op_abi.STATE

NAMES = {op_abi: ("sextans_edge_op_device_rm_bf16", "sextans_edge_op_backward_device_rm_bf16"),
         edge_abi: ("sextans_spmm_edge_device_rm_bf16", "sextans_spmm_edge_backward_device_rm_bf16")}


def test_symbols_exported(sx):
    from sextans_amd import api
    api.lib()
    raw = C.CDLL(api.LIB_PATH)
    for pair in NAMES.values():
        for name in pair:
            assert name in api._OPTIONAL_SYMBOLS and hasattr(raw, name), name


@pytest.mark.parametrize("fake", [False, True])
@pytest.mark.parametrize("family", ["edge_op", "spmm_edge"])
def test_every_refusal_of_the_fp32_twin_in_its_order(sx, monkeypatch, family, fake):
    """bad op, bad N, bad and optional leading dimensions, misalignment, nothing to compute, a gradient of an unread operand, COPY with
    dB, then the handle's state: the twin's own test, pointed at the bf16 names"""
    mod = op_abi if family == "edge_op" else edge_abi
    monkeypatch.setattr(mod, "FWD_NAME", NAMES[mod][0])
    monkeypatch.setattr(mod, "BWD_NAME", NAMES[mod][1])
    mod.test_argument_checks(sx, fake)


def test_the_order_of_the_checks_on_a_handle_without_a_matrix(sx):
    """the argument errors come before the state: each is INVALID on a zeroed handle, on which a valid call is STATE"""
    from sextans_amd import api
    L = api.lib()
    h = (C.c_char * (1 << 20))()
    hp = C.addressof(h)
    f, b = NAMES[op_abi]
    assert op_abi.call(L, f, hp, op_abi.FWD) == STATE and op_abi.call(L, b, hp, op_abi.BWD) == STATE
    for over in (dict(op=9), dict(N=12), dict(lde=18), dict(ldz=8), dict(E=50), dict(Z=66)):   # (bf16 pointers too are 16-byte aligned)
        assert op_abi.call(L, f, hp, op_abi.FWD, **over) == INVALID, over
    for over in (dict(op=0), dict(N=4), dict(ldgz=18), dict(Gz=50), dict(dxdst=0, dxsrc=0), dict(op=op_abi.DST), dict(op=op_abi.SRC)):
        assert op_abi.call(L, b, hp, op_abi.BWD, **over) == INVALID, over
    f, b = NAMES[edge_abi]
    assert edge_abi.call(L, f, hp, edge_abi.FWD) == STATE and edge_abi.call(L, b, hp, edge_abi.BWD) == STATE
    for over in (dict(op=5), dict(N=20), dict(lde=18), dict(E=50)):
        assert edge_abi.call(L, f, hp, edge_abi.FWD, **over) == INVALID, over
    for over in (dict(op=5), dict(ldde=18), dict(dE=114), dict(dB=0, dE=0), dict(op=edge_abi.COPY)):
        assert edge_abi.call(L, b, hp, edge_abi.BWD, **over) == INVALID, over
    # a required pointer that is NULL comes after the state
    assert op_abi.call(L, NAMES[op_abi][0], hp, op_abi.FWD, Z=0) == STATE
    assert op_abi.call(L, NAMES[op_abi][1], hp, op_abi.BWD, Gz=0) == STATE
    assert edge_abi.call(L, NAMES[edge_abi][0], hp, edge_abi.FWD, E=0) == STATE


def test_python_and_torch_surfaces(sx):
    from sextans_amd import api, edge_op, edge_op_bf16
    for twin in ("edge_op_device_rm", "edge_op_backward_device_rm", "spmm_edge_device_rm", "spmm_edge_backward_device_rm"):
        a, b = (inspect.signature(getattr(api.Engine, name)).parameters for name in (twin, twin + "_bf16"))
        assert list(a) == list(b) and b["stream"].default is None, twin
    # the bf16 route of the torch op: a function of its own with edge_op()'s parameter list (which stays what it is)
    assert inspect.signature(edge_op_bf16.edge_op_bf16) == inspect.signature(edge_op.edge_op)
    assert edge_op_bf16.__all__ == ["edge_op_bf16"] and "edge_op_bf16" in edge_op.edge_op.__doc__
    with pytest.raises(ValueError):   # (an unknown op is refused before anything else is looked at, as in edge_op())
        edge_op_bf16.edge_op_bf16(None, op="div")
    with open(os.path.join(ROOT, "include", "sextans_amd.h")) as f:
        text = " ".join(f.read().split())
    assert ("int sextans_edge_op_device_rm_bf16(sextans_handle_t h, int op, int N, const float *d_xdst, int64_t ldxdst, const float *d_xsrc, "
            "int64_t ldxsrc, const uint16_t *d_E, int64_t lde, uint16_t *d_Z, int64_t ldz, void *stream);") in text
    assert ("int sextans_edge_op_backward_device_rm_bf16(sextans_handle_t h, int op, int N, const float *d_xdst, int64_t ldxdst, "
            "const float *d_xsrc, int64_t ldxsrc, const uint16_t *d_Gz, int64_t ldgz, float *d_dxdst, int64_t lddxdst, float *d_dxsrc, "
            "int64_t lddxsrc, void *stream);") in text
    assert ("int sextans_spmm_edge_device_rm_bf16(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const uint16_t *d_E, "
            "int64_t lde, float *d_C, int64_t ldc, void *stream);") in text
    assert ("int sextans_spmm_edge_backward_device_rm_bf16(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, "
            "const uint16_t *d_E, int64_t lde, const float *d_G, int64_t ldg, float *d_dB, int64_t lddb, uint16_t *d_dE, int64_t ldde, "
            "void *stream);") in text


def round_rule(u32):
    """the header's rule on fp32 bit patterns: NaN -> a quiet NaN with its sign and upper payload, everything else the integer round to
    nearest even, whose carry runs into the exponent"""
    u = np.asarray(u32, np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    rounded = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u >> 16) | 0x40, rounded).astype(np.uint16)


# fp32 bit patterns -> the bf16 bit pattern the contract asks for
FIXED = [
    (0x3F808000, 0x3F80),   # 1 + 2^-8: a tie, down to the even 1.0
    (0x3F818000, 0x3F82),   # a tie, up to the even neighbour
    (0x3F808001, 0x3F81),   # just above a tie: up
    (0x3F817FFF, 0x3F81),   # just below a tie: down
    (0xBF808000, 0xBF80), (0xBF818000, 0xBF82),   # the same ties, negative
    (0x7F7FFFFF, 0x7F80),   # the largest finite fp32: inf
    (0x7F7F8000, 0x7F80),   # the rounding boundary itself (a tie whose even neighbour is inf): inf
    (0x7F7F7FFF, 0x7F7F),   # just below it: the largest finite bf16
    (0xFF7FFFFF, 0xFF80),
    (0x00000001, 0x0000),   # the smallest denormal: +0
    (0x00008000, 0x0000),   # a denormal tie: down to the even +0
    (0x00008001, 0x0001),   # a denormal just above it: the smallest bf16 denormal
    (0x00018000, 0x0002),   # a denormal tie: up to the even neighbour
    (0x007FFFFF, 0x0080),   # the largest denormal: the smallest normal
    (0x807FFFFF, 0x8080),
    (0x00000000, 0x0000), (0x80000000, 0x8000),   # +-0
    (0x7F800000, 0x7F80), (0xFF800000, 0xFF80),   # +-inf
]
NANS = [0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF, 0x7F80FFFF, 0xFFFFFFFF]


def test_host_rounding_is_the_contract_on_fixed_values():
    from test_bf16_operands_gpu import same16, to_bf16, widen
    bits = np.array([b for b, _ in FIXED], np.uint32)
    want = np.array([w for _, w in FIXED], np.uint16)
    assert np.array_equal(round_rule(bits), want)                      # the rule restated here gives the table
    got = to_bf16(bits.view(np.float32))
    assert np.array_equal(got, want), [(hex(b), hex(g), hex(w)) for b, g, w in zip(bits, got, want) if g != w]
    nan = to_bf16(np.array(NANS, np.uint32).view(np.float32))
    assert np.all(np.isnan(widen(nan))) and same16(nan, round_rule(NANS))   # a NaN stays a NaN (compared as NaN, as same16 does)
    assert np.all(np.isnan(widen(round_rule(NANS)))) and np.all(round_rule(NANS) & 0x40)   # ... a quiet one by the rule
    # widening is exact and rounding a widened value gives it back
    every = np.arange(0, 1 << 16, 7, dtype=np.uint16)
    every = every[~np.isnan(widen(every))]
    assert np.array_equal(to_bf16(widen(every)), every) and np.array_equal(round_rule(widen(every).view(np.uint32)), every)
