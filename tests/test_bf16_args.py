"""bf16 dense operands (sextans_spmm_device_rm_bf16, sextans_spmm_t_device_rm_bf16, sextans_prepare_rm_bf16): the library exports them,
the Python and torch surfaces expose them, and bad arguments are refused with error codes before any device is touched -- every argument
check first, then SEXTANS_ERR_STATE, and only then the first HIP call (no GPU needed)."""
import ctypes as C
import inspect
import os

from util import ROOT

INVALID = 9
STATE = 12
F32, BF16 = 0, 1


def test_bf16_entry_points_reject_bad_arguments(sx):
    from sextans_amd import api
    L = api.lib()
    raw = C.CDLL(api.LIB_PATH)
    for name in ("sextans_spmm_device_rm_bf16", "sextans_spmm_t_device_rm_bf16", "sextans_prepare_rm_bf16"):
        assert name in api._OPTIONAL_SYMBOLS and hasattr(raw, name), name
    # A handle without a matrix (zeroed engine state): valid arguments pass every check and stop at SEXTANS_ERR_STATE before anything
    # touches a device, so each bad argument below is refused by its own check.
    h = (C.c_char * (1 << 20))()
    hp = C.addressof(h)
    for f in (L.sextans_spmm_device_rm_bf16, L.sextans_spmm_t_device_rm_bf16):
        # (h, N, alpha, B, ldb, beta, C_in, ldc_in, C_out, ldc, c_dtype, stream); pointers are plain numbers, never dereferenced
        ok = dict(h=hp, N=16, alpha=1.0, B=32, ldb=16, beta=0.0, Cin=64, ldc_in=16, Cout=96, ldc=16, dt=F32, s=None)

        def call(**kw):
            a = dict(ok, **kw)
            return f(a["h"], a["N"], a["alpha"], a["B"], a["ldb"], a["beta"], a["Cin"], a["ldc_in"], a["Cout"], a["ldc"], a["dt"], a["s"])

        assert call() == STATE
        assert call(dt=BF16) == STATE
        assert call(B=34, Cin=66, Cout=98, dt=BF16) == STATE            # 2-byte aligned bf16 operands are valid (they convert)
        assert call(B=34, Cin=68, Cout=100) == STATE                    # ... and 4-byte aligned fp32 C
        assert call(Cin=96) == STATE                                    # C_in may alias C_out
        assert call(ldb=24, ldc_in=20, ldc=28) == STATE                 # padded leading dimensions
        assert call(h=None) == INVALID
        assert call(N=12) == INVALID                                    # N % 8
        assert call(N=0) == INVALID
        assert call(B=None) == INVALID
        assert call(Cin=None) == INVALID
        assert call(Cout=None) == INVALID
        assert call(ldb=8) == INVALID                                   # ldb < N
        assert call(ldc_in=8) == INVALID
        assert call(ldc=8) == INVALID
        assert call(B=33) == INVALID                                    # odd address of a bf16 B
        assert call(Cin=65, dt=BF16) == INVALID                         # odd address of a bf16 C
        assert call(Cout=97, dt=BF16) == INVALID
        assert call(Cin=66) == INVALID                                  # fp32 C not on a 4-byte boundary
        assert call(Cout=98) == INVALID
        for dt in (2, -1):
            assert call(dt=dt) == INVALID, dt
    P = L.sextans_prepare_rm_bf16
    assert P(hp, 16, F32, 0, None) == STATE
    assert P(hp, 16, BF16, 1, None) == STATE
    assert P(None, 16, F32, 0, None) == INVALID
    assert P(hp, 12, F32, 0, None) == INVALID
    assert P(hp, 0, F32, 0, None) == INVALID
    for dt in (2, -1):
        assert P(hp, 16, dt, 0, None) == INVALID, dt
    for tr in (2, -1):
        assert P(hp, 16, F32, tr, None) == INVALID, tr
    # sextans_prepare keeps refusing the unused layout constants: the bf16 form is a function of its own, not a layout
    for layout in (2, 4, -1):
        assert L.sextans_prepare(hp, 16, layout, None) == INVALID, layout


def test_python_and_torch_surfaces():
    from sextans_amd import api, torch_op
    for name in ("spmm_device_rm_bf16", "spmm_t_device_rm_bf16", "prepare_rm_bf16"):
        assert callable(getattr(api.Engine, name)), name
    assert (api.DTYPE_F32, api.DTYPE_BF16) == (0, 1)
    sig = inspect.signature(api.Engine.prepare_rm_bf16).parameters
    assert list(sig)[1:] == ["N", "c_dtype", "transposed", "stream"] and sig["transposed"].default is False
    assert inspect.signature(api.Engine.spmm_device_rm_bf16).parameters["c_dtype"].default == api.DTYPE_F32
    sig = inspect.signature(torch_op.spmm)
    assert sig.parameters["out_dtype"].default is None
    assert sig.parameters["transpose_a"].default is False
    with open(os.path.join(ROOT, "include", "sextans_amd.h")) as f:
        text = f.read()
    assert "#define SEXTANS_DTYPE_F32 0" in text and "#define SEXTANS_DTYPE_BF16 1" in text
