"""The backward-pass entry points on a LIVE handle with a matrix set: every argument rule of sextans_sddmm_device_rm (no fallback: its
loads and stores are 16-byte vectors), sextans_spmm_t_device_rm and sextans_prepare is enforced by its own check, while the same call
with valid arguments succeeds."""
import numpy as np
import pytest

from util import random_csr

pytestmark = pytest.mark.gpu

INVALID = 9


def test_live_handle_rejects_each_bad_argument(sx):
    import torch
    from sextans_amd import api
    rs = np.random.RandomState(1)
    M, K, N = 300, 200, 16
    rp, ci, v = random_csr(rs, M, K, 5)
    X = torch.zeros(M * N + 64, device="cuda"); Y = torch.zeros(K * N + 64, device="cuda")
    vin = torch.zeros(len(ci) + 64, device="cuda"); vout = torch.zeros(len(ci) + 64, device="cuda")
    B = torch.zeros(M * N + 64, device="cuda"); C = torch.zeros(K * N + 64, device="cuda")
    x, y, i, o, b, c = (t.data_ptr() for t in (X, Y, vin, vout, B, C))
    st = torch.cuda.current_stream().cuda_stream
    L = api.lib()
    with sx.Engine(0) as e:
        e.set_matrix_csr(M, K, rp, ci, v)
        h = e._h
        assert L.sextans_sddmm_device_rm(h, N, 1.0, x, N, y, N, 0.5, i, o, st) == 0
        assert L.sextans_spmm_t_device_rm(h, N, 1.0, b, N, 0.0, c, N, c, N, st) == 0
        assert L.sextans_prepare(h, N, 3, st) == 0
        bad_sddmm = [(12, x, N, y, N, i, o), (N, x, 8, y, N, i, o), (N, x, N, y, 8, i, o), (N, x, 18, y, N, i, o), (N, x, N, y, 18, i, o),
                     (N, x + 4, N, y, N, i, o), (N, x, N, y + 4, N, i, o), (N, x, N, y, N, i + 8, o), (N, x, N, y, N, i, o + 4),
                     (N, x, N, y, N, i, None)]
        for n, xx, lx, yy, ly, ii, oo in bad_sddmm:
            assert L.sextans_sddmm_device_rm(h, n, 1.0, xx, lx, yy, ly, 0.5, ii, oo, st) == INVALID, (n, lx, ly)
        for n, lb, lci, lc in ((12, N, N, N), (N, 8, N, N), (N, N, 8, N), (N, N, N, 8)):
            assert L.sextans_spmm_t_device_rm(h, n, 1.0, b, lb, 0.0, c, lci, c, lc, st) == INVALID, (n, lb, lci, lc)
        for layout in (2, 4):
            assert L.sextans_prepare(h, N, layout, st) == INVALID, layout
        assert L.sextans_prepare(h, 12, 3, st) == INVALID
        torch.cuda.synchronize()
