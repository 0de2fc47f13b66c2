"""sextans_sddmm_device_rm: out[e] = alpha * sum_n X[r, n] * Y[c, n] (+ beta * in[e]) for every entry e = (r, c) of A in CSR order,
every product and every sum rounded to fp32 in column order -- bit-identical to the numpy restatement below (numpy rounds each float32
product and each float32 sum separately)."""
import numpy as np
import pytest

from util import random_csr

pytestmark = pytest.mark.gpu


def sddmm_ref(rp, ci, X, Y, alpha, beta=0.0, vin=None):
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    cols = np.asarray(ci, np.int64)
    acc = np.zeros(len(ci), np.float32)
    with np.errstate(all="ignore"):
        for n in range(X.shape[1]):
            acc = acc + (X[rows, n] * Y[cols, n])
        out = np.float32(alpha) * acc
        if vin is not None:
            out = out + np.float32(beta) * vin
    return out.astype(np.float32)


def run(e, X, Y, alpha, beta=0.0, vin=None, alias=False, ldx=None, ldy=None):
    import torch
    (M, N), K = X.shape, Y.shape[0]
    ldx, ldy = ldx or N, ldy or N
    dX = torch.full((M, ldx), float("nan"), device="cuda"); dX[:, :N] = torch.from_numpy(X).cuda()
    dY = torch.full((K, ldy), float("nan"), device="cuda"); dY[:, :N] = torch.from_numpy(Y).cuda()
    nnz = e.nnz
    dout = torch.full((max(nnz, 1),), -9.0, device="cuda")
    din = None
    if vin is not None:
        din = dout if alias else torch.from_numpy(vin).cuda()
        if alias:
            dout[:nnz] = torch.from_numpy(vin).cuda()
    st = torch.cuda.current_stream().cuda_stream
    e.sddmm_device_rm(N, alpha, dX.data_ptr(), ldx, dY.data_ptr(), ldy, beta, din.data_ptr() if din is not None else None,
                      dout.data_ptr(), st)
    torch.cuda.synchronize()
    return dout.cpu().numpy()[:nnz]


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("N", [8, 16, 24, 64, 128])
def test_random_matrix_all_input_forms(sx, N):
    rs = np.random.RandomState(N)
    M, K = 3000, 2200
    rp, ci, v = random_csr(rs, M, K, 11, empty_frac=0.1, long_rows=2)
    X = rs.uniform(-1, 1, (M, N)).astype(np.float32); Y = rs.uniform(-1, 1, (K, N)).astype(np.float32)
    vin = rs.uniform(-1, 1, len(ci)).astype(np.float32)
    with sx.Engine(0) as e:
        e.set_matrix_csr(M, K, rp, ci, v)
        assert same(run(e, X, Y, 0.85), sddmm_ref(rp, ci, X, Y, 0.85))
        assert e.last_kernel().startswith("sddmm_rowmajor")
        assert same(run(e, X, Y, 0.85, -2.06, vin), sddmm_ref(rp, ci, X, Y, 0.85, -2.06, vin))
        assert same(run(e, X, Y, 0.85, -2.06, vin, alias=True), sddmm_ref(rp, ci, X, Y, 0.85, -2.06, vin))
        assert same(run(e, X, Y, 1.0, ldx=N + 4, ldy=N + 12), sddmm_ref(rp, ci, X, Y, 1.0))


def test_hub_row_rectangular_and_nonfinite(sx):
    rs = np.random.RandomState(9)
    M, K, N = 700, 250000, 16
    lens = rs.poisson(5, M); lens[0] = lens[M // 2] = 0; lens[17] = 200000
    rp = np.zeros(M + 1, np.int32); rp[1:] = np.cumsum(lens)
    ci = np.concatenate([np.sort(rs.choice(K, n, replace=False)) for n in lens]).astype(np.int32)
    v = rs.uniform(-1, 1, len(ci)).astype(np.float32)
    X = rs.uniform(-1, 1, (M, N)).astype(np.float32); Y = rs.uniform(-1, 1, (K, N)).astype(np.float32)
    X[3, 5] = np.inf; X[17, 0] = -np.inf                   # inf * 0 = NaN where Y is 0, +-inf elsewhere
    Y[ci[rp[17]:rp[17] + 50], 0] = 0.0
    with sx.Engine(0) as e:
        e.set_matrix_csr(M, K, rp, ci, v)
        assert same(run(e, X, Y, 0.5), sddmm_ref(rp, ci, X, Y, 0.5))
    # a wide matrix (K << M) as well
    M2, K2 = 5000, 40
    rp2, ci2, v2 = random_csr(rs, M2, K2, 6)
    X2 = rs.uniform(-1, 1, (M2, 32)).astype(np.float32); Y2 = rs.uniform(-1, 1, (K2, 32)).astype(np.float32)
    with sx.Engine(0) as e:
        e.set_matrix_csr(M2, K2, rp2, ci2, v2)
        assert same(run(e, X2, Y2, 2.0), sddmm_ref(rp2, ci2, X2, Y2, 2.0))


def test_entry_order_after_a_clustered_plan(sx):
    """The output follows the CSR order the matrix was set with, also after a forward call built a graph-clustered plan."""
    import torch
    from sextans_amd import api, meshgen
    rp, ci, v = api.gen_fem3d_host(24, 22, 20, 3, 7)
    M = K = 24 * 22 * 20 * 3
    rp, ci, v = meshgen.permute_symmetric(rp, ci, v, M, meshgen.node_permutation(M // 3, 3, 9))
    N = 16
    rs = np.random.RandomState(3)
    X = rs.uniform(-1, 1, (M, N)).astype(np.float32); Y = rs.uniform(-1, 1, (K, N)).astype(np.float32)
    with sx.Engine(0) as e:
        e.set_matrix_csr(M, K, rp, ci, v)
        e.set_option("row_cluster", 2)
        dB = torch.from_numpy(Y).cuda(); dC = torch.zeros((M, N), device="cuda")
        e.spmm_device_rm(N, 1.0, dB.data_ptr(), N, 0.0, dC.data_ptr(), N, dC.data_ptr(), N, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert e.get_stat("row_cluster") != 0, e.last_kernel()   # the clustered plan was evaluated (and built: 1 / 2)
        assert same(run(e, X, Y, 1.0), sddmm_ref(rp, ci, X, Y, 1.0))
