"""Stat "device_bytes" is the sum of what the engine's device buffers asked the runtime for (device_buffer.h: DevBuf::bytes()), so it
can be checked as a measurement:
  - the same matrix and the same calls give the same count -- a buffer counted twice, or one that survives the matrix uncounted and is
    allocated again, shows as a difference;
  - a matrix that is rejected leaves nothing behind;
  - the count is at least the terms include/sextans_amd.h documents: the owned matrix, A^T with its permutation, the softmax table.
Everything goes through api.Engine."""
import os

import numpy as np
import pytest

from util import CASES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NASA = os.path.join(ROOT, "matrices", "nasa4704", "nasa4704.mtx")
N = 16
INDEX = 6   # SEXTANS_ERR_INDEX


def load(sx, path):
    rp, ci, v, M, K, nnz = sx.read_suitsparse_matrix(path)
    return np.asarray(rp, np.int32), np.asarray(ci, np.int32), np.asarray(v, np.float32), M, K


def calls(e, M, K, nnz, lanes=(0,)):
    """A column-major SpMM (once per lanes_per_row value), a row-major one, a transposed row-major one, a row softmax and a value
    refresh from a device array, on the matrix that is set."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(5)
    rnd = lambda *shape: torch.rand(*shape, device="cuda", generator=g) - 0.5
    s = torch.cuda.current_stream().cuda_stream
    B, C = rnd(K * N), rnd(M * N)
    for lpr in lanes:
        e.set_option("lanes_per_row", lpr)
        e.spmm_device(N, 1.0, B.data_ptr(), K, 0.5, C.data_ptr(), C.data_ptr(), M, s)
    e.spmm_device_rm(N, 1.0, B.data_ptr(), N, 0.5, C.data_ptr(), N, C.data_ptr(), N, s)
    Bt, Ct = rnd(M * N), rnd(K * N)
    e.spmm_t_device_rm(N, 1.0, Bt.data_ptr(), N, 0.5, Ct.data_ptr(), N, Ct.data_ptr(), N, s)
    x, p = rnd(max(nnz, 4)), torch.empty(max(nnz, 4), device="cuda")
    e.row_softmax_device(0.125, x.data_ptr(), p.data_ptr(), s)
    e.update_values_device(x.data_ptr(), s)
    torch.cuda.synchronize()
    return e.get_stat("device_bytes")


def test_same_work_same_count_nasa4704(sx):
    rp, ci, v, M, K = load(sx, NASA)
    with sx.Engine(0) as e:
        e.set_matrix_csr(M, K, rp, ci, v)
        b1 = calls(e, M, K, len(ci))
        e.set_matrix_csr(M, K, rp, ci, v)
        b2 = calls(e, M, K, len(ci))
        print("device_bytes nasa4704:", b1, b2)
        assert b2 == b1
        # ... and it is at least what the header documents: the owned matrix, A^T and its permutation, the softmax table
        assert b1 >= (M + 1) * 4 + len(ci) * 8 + (K + 1) * 4 + len(ci) * 12 + len(ci) // 64


def test_same_work_same_count_piece_path_and_plan_stash(sx):
    rp, ci, v, M, K = load(sx, os.path.join(CASES, "empty_rows_long_row.mtx"))
    with sx.Engine(0) as e:
        e.set_option("bucket_rows", 4)   # the rows above 4 entries (a third of the non-empty ones, the 228-entry row among them) take the piece path
        e.set_option("kernel", 2)        # a packed plan per lane count, whatever the sampled reuse says: 2, 4, 2 parks and brings back plans
        e.set_matrix_csr(M, K, rp, ci, v)
        b1 = calls(e, M, K, len(ci), lanes=(2, 4, 2))
        assert e.get_stat("piece_path_rows") > 0
        e.set_matrix_csr(M, K, rp, ci, v)
        b2 = calls(e, M, K, len(ci), lanes=(2, 4, 2))
        print("device_bytes empty_rows_long_row:", b1, b2)
        assert b2 == b1


def test_rejected_matrix_leaves_nothing_behind(sx):
    import torch
    rp, ci, v, M, K = load(sx, NASA)
    with sx.Engine(0) as e:
        e.set_matrix_csr(M, K, rp, ci, v)
        b = calls(e, M, K, len(ci))
        # 2 x 5 with a column index of 700: the validation kernel rejects it before anything is gathered
        d_rp = torch.tensor([0, 2, 3], dtype=torch.int32, device="cuda")
        d_ci = torch.tensor([0, 700, 2], dtype=torch.int32, device="cuda")
        d_v = torch.ones(3, device="cuda")
        e.set_matrix_csr_device(2, 5, 3, d_rp.data_ptr(), d_ci.data_ptr(), d_v.data_ptr())
        B, C = torch.ones(5 * 8, device="cuda"), torch.zeros(2 * 8, device="cuda")
        with pytest.raises(sx.api.SextansError) as err:
            e.spmm_device(8, 1.0, B.data_ptr(), 5, 0.0, C.data_ptr(), C.data_ptr(), 2, torch.cuda.current_stream().cuda_stream)
        assert err.value.code == INDEX
        e.set_matrix_csr(M, K, rp, ci, v)
        after = calls(e, M, K, len(ci))
        print("device_bytes before / after a rejected matrix:", b, after)
        assert after == b
