"""Backward-pass entry points (sextans_csr_transpose_device, sextans_spmm_t_device_rm, sextans_sddmm_device_rm, sextans_prepare with
SEXTANS_LAYOUT_ROWMAJOR_T): bad arguments are refused with error codes before any device is touched (no GPU needed), and the Python and
torch surfaces expose them."""
import ctypes as C
import inspect
import os

from util import ROOT

INVALID = 9
STATE = 12


def test_backward_entry_points_reject_bad_arguments(sx):
    from sextans_amd import api
    L = api.lib()
    raw = C.CDLL(api.LIB_PATH)
    for name in ("sextans_csr_transpose_device", "sextans_spmm_t_device_rm", "sextans_sddmm_device_rm"):
        assert name in api._OPTIONAL_SYMBOLS and hasattr(raw, name), name
    # NULL handle
    assert L.sextans_spmm_t_device_rm(None, 16, 1.0, 16, 16, 0.0, 16, 16, 16, 16, None) == INVALID
    assert L.sextans_sddmm_device_rm(None, 16, 1.0, 16, 16, 16, 16, 0.0, None, 16, None) == INVALID
    assert L.sextans_prepare(None, 16, 3, None) == INVALID
    # A handle without a matrix (zeroed engine state: no matrix set): valid arguments pass every check and stop at
    # SEXTANS_ERR_STATE before anything touches a device, so each bad argument below is refused by its own check.
    h = (C.c_char * (1 << 20))()
    hp = C.addressof(h)
    assert L.sextans_spmm_t_device_rm(hp, 16, 1.0, 16, 16, 0.0, 16, 16, 16, 16, None) == STATE
    assert L.sextans_sddmm_device_rm(hp, 16, 1.0, 16, 16, 32, 16, 0.0, 48, 64, None) == STATE
    assert L.sextans_sddmm_device_rm(hp, 16, 1.0, 16, 16, 32, 16, 0.0, None, 64, None) == STATE    # vals_in NULL is allowed
    assert L.sextans_prepare(hp, 16, 3, None) == STATE
    assert L.sextans_spmm_t_device_rm(hp, 12, 1.0, 16, 16, 0.0, 16, 16, 16, 16, None) == INVALID    # N % 8
    assert L.sextans_spmm_t_device_rm(hp, 16, 1.0, 16, 8, 0.0, 16, 16, 16, 16, None) == INVALID     # ldb < N
    assert L.sextans_spmm_t_device_rm(hp, 16, 1.0, 16, 16, 0.0, 16, 8, 16, 16, None) == INVALID     # ldc_in < N
    assert L.sextans_spmm_t_device_rm(hp, 16, 1.0, 16, 16, 0.0, 16, 16, 16, 8, None) == INVALID     # ldc < N
    assert L.sextans_sddmm_device_rm(hp, 12, 1.0, 16, 16, 32, 16, 0.0, 48, 64, None) == INVALID     # N % 8
    assert L.sextans_sddmm_device_rm(hp, 16, 1.0, 16, 8, 32, 16, 0.0, 48, 64, None) == INVALID      # ldx < N
    assert L.sextans_sddmm_device_rm(hp, 16, 1.0, 16, 16, 32, 8, 0.0, 48, 64, None) == INVALID      # ldy < N
    assert L.sextans_sddmm_device_rm(hp, 16, 1.0, 16, 18, 32, 16, 0.0, 48, 64, None) == INVALID     # ldx % 4
    assert L.sextans_sddmm_device_rm(hp, 16, 1.0, 16, 16, 32, 18, 0.0, 48, 64, None) == INVALID     # ldy % 4
    assert L.sextans_sddmm_device_rm(hp, 16, 1.0, 20, 16, 32, 16, 0.0, 48, 64, None) == INVALID     # X 4 bytes off
    assert L.sextans_sddmm_device_rm(hp, 16, 1.0, 16, 16, 36, 16, 0.0, 48, 64, None) == INVALID     # Y 4 bytes off
    assert L.sextans_sddmm_device_rm(hp, 16, 1.0, 16, 16, 32, 16, 0.0, 56, 64, None) == INVALID     # vals_in 8 bytes off
    assert L.sextans_sddmm_device_rm(hp, 16, 1.0, 16, 16, 32, 16, 0.0, 48, 68, None) == INVALID     # vals_out 4 bytes off
    assert L.sextans_sddmm_device_rm(hp, 16, 1.0, 16, 16, 32, 16, 0.0, 48, None, None) == INVALID   # no output
    for layout in (2, 4, -1):
        assert L.sextans_prepare(hp, 16, layout, None) == INVALID, layout
    assert L.sextans_prepare(hp, 12, 3, None) == INVALID
    # the transpose: negative sizes, entries without rows, missing outputs
    p, i, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
    out = (C.byref(p), C.byref(i), C.byref(v))
    assert L.sextans_csr_transpose_device(0, -1, 4, 0, 16, 16, 16, *out, None) == INVALID
    assert L.sextans_csr_transpose_device(0, 4, 4, -1, 16, 16, 16, *out, None) == INVALID
    assert L.sextans_csr_transpose_device(0, 0, 4, 3, 16, 16, 16, *out, None) == INVALID
    assert L.sextans_csr_transpose_device(0, 4, 4, 3, None, 16, 16, *out, None) == INVALID
    assert L.sextans_csr_transpose_device(0, 4, 4, 3, 16, 16, 16, None, None, None, None) == INVALID
    assert L.sextans_csr_transpose_device(0, 4, 4, 1 << 31, 16, 16, 16, *out, None) == INVALID


def test_python_and_torch_surfaces():
    from sextans_amd import api, torch_op
    for name in ("spmm_t_device_rm", "sddmm_device_rm"):
        assert callable(getattr(api.Engine, name)), name
    assert "transposed" in inspect.signature(api.Engine.prepare).parameters
    assert callable(api.csr_transpose_device)
    sig = inspect.signature(torch_op.spmm)
    assert sig.parameters["transpose_a"].default is False
    with open(os.path.join(ROOT, "include", "sextans_amd.h")) as f:
        assert "#define SEXTANS_LAYOUT_ROWMAJOR_T 3" in f.read()
