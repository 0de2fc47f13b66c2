"""Row softmax on A's pattern (sextans_row_softmax_device, sextans_row_softmax_backward_device): the symbols exist, bad arguments and a
handle without a matrix are refused with error codes before any device is touched (no GPU needed), and the Python surfaces expose them."""
import ctypes as C
import inspect
import os

from util import ROOT

INVALID = 9
STATE = 12


def test_row_softmax_symbols_and_argument_checks(sx):
    from sextans_amd import api
    L = api.lib()
    raw = C.CDLL(api.LIB_PATH)
    for name in ("sextans_row_softmax_device", "sextans_row_softmax_backward_device"):
        assert name in api._OPTIONAL_SYMBOLS and hasattr(raw, name), name
    # NULL handle
    assert L.sextans_row_softmax_device(None, 1.0, 16, 16, None) == INVALID
    assert L.sextans_row_softmax_backward_device(None, 1.0, 16, 16, 16, None) == INVALID
    h = (C.c_char * (1 << 20))()   # a handle without a matrix (zeroed engine state)
    hp = C.addressof(h)
    # misaligned pointers: INVALID whatever the state; aligned ones on a handle without a CSR matrix: STATE, before any device is touched
    assert L.sextans_row_softmax_device(hp, 1.0, 20, 16, None) == INVALID
    assert L.sextans_row_softmax_device(hp, 1.0, 16, 24, None) == INVALID
    assert L.sextans_row_softmax_backward_device(hp, 1.0, 16, 16, 36, None) == INVALID
    assert L.sextans_row_softmax_device(hp, 1.0, 16, 16, None) == STATE
    assert L.sextans_row_softmax_backward_device(hp, 1.0, 16, 32, 48, None) == STATE


def test_python_and_torch_surfaces():
    from sextans_amd import api, torch_op
    for name in ("row_softmax_device", "row_softmax_backward_device"):
        assert callable(getattr(api.Engine, name)), name
        assert inspect.signature(getattr(api.Engine, name)).parameters["stream"].default is None
    assert list(inspect.signature(api.Engine.row_softmax_device).parameters)[1:] == ["scale", "d_x", "d_p", "stream"]
    assert list(inspect.signature(api.Engine.row_softmax_backward_device).parameters)[1:] == ["scale", "d_p", "d_g", "d_dx", "stream"]
    for name in ("sddmm", "row_softmax", "sparse_attention"):
        assert callable(getattr(torch_op, name)), name
    sig = inspect.signature(torch_op.sparse_attention).parameters
    assert sig["scale"].default is None and sig["bias"].default is False
    with open(os.path.join(ROOT, "include", "sextans_amd.h")) as f:
        text = f.read()
    assert "int sextans_row_softmax_device(sextans_handle_t h, float scale, const float *d_x, float *d_p, void *stream);" in text
    assert ("int sextans_row_softmax_backward_device(sextans_handle_t h, float scale, const float *d_p, const float *d_g, float *d_dx, "
            "void *stream);") in text.replace("\n", " ").replace("  ", " ")
