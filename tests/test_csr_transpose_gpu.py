"""sextans_csr_transpose_device: the CSR of A^T, byte-identical to the reference's CSC_2_CSR of A's CSR read as the CSC of A^T
(oracle.csc_to_csr(K, M, row_ptr, col_idx, val)), deterministic."""
import glob
import os

import numpy as np
import pytest

from util import CASES, NASA, random_csr

pytestmark = pytest.mark.gpu


def device_transpose(M, K, rp, ci, v):
    import torch
    from sextans_amd import api
    nnz = len(ci)
    drp = torch.from_numpy(np.asarray(rp, np.int32)).cuda()
    dci = torch.from_numpy(np.asarray(ci, np.int32) if nnz else np.zeros(1, np.int32)).cuda()
    dv = torch.from_numpy(np.asarray(v, np.float32) if nnz else np.zeros(1, np.float32)).cuda()
    p, i, x = api.csr_transpose_device(0, M, K, nnz, drp.data_ptr(), dci.data_ptr(), dv.data_ptr())
    out = []
    for ptr, n, dt in ((p, K + 1, np.int32), (i, nnz, np.int32), (x, nnz, np.float32)):
        a = np.zeros(max(n, 1), dt)
        api.device_copy(0, a.ctypes.data, ptr, n * 4, api.COPY_D2H)
        api.device_free(0, ptr)
        out.append(a[:n])
    return out


def check(oracle, M, K, rp, ci, v):
    want = oracle.csc_to_csr(K, M, np.asarray(rp, np.int32), np.asarray(ci, np.int32), np.asarray(v, np.float32))
    got = device_transpose(M, K, rp, ci, v)
    for g, w, what in zip(got, want, ("row_ptr", "col_idx", "val")):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), what
    return got


def test_golden_matrices_and_nasa4704(sx, oracle):
    paths = sorted(glob.glob(os.path.join(CASES, "*.mtx"))) + [NASA]
    assert len(paths) >= 16
    for path in paths:
        rp, ci, v, M, K, nnz = sx.read_suitsparse_matrix(path)
        check(oracle, M, K, rp, ci, v)


def test_random_duplicates_rectangular_and_empty(sx, oracle):
    rs = np.random.RandomState(5)
    for M, K in ((3000, 3000), (4000, 1500), (1200, 5000)):       # square, tall, wide; empty rows and columns
        rp, ci, v = random_csr(rs, M, K, 6, empty_frac=0.2)
        check(oracle, M, K, rp, ci, v)
    # duplicate (row, column) entries and unsorted columns: storage order is kept inside each row of A^T
    rp = np.array([0, 4, 4, 7], np.int32)
    ci = np.array([2, 0, 2, 2, 1, 0, 1], np.int32)
    v = np.arange(1, 8, dtype=np.float32)
    got = check(oracle, 3, 4, rp, ci, v)
    assert got[2][got[0][2]:got[0][3]].tolist() == [1.0, 3.0, 4.0]
    check(oracle, 5, 7, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))   # nnz = 0
    check(oracle, 0, 6, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))   # M = 0


def test_powerlaw_and_determinism(sx, oracle):
    M = K = 60000
    rp, ci, v = sx.api.gen_powerlaw_host(M, K, 4, 120, 30000, 11)
    first = check(oracle, M, K, rp, ci, v)
    again = device_transpose(M, K, rp, ci, v)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
