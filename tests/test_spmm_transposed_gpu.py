"""sextans_spmm_t_device_rm: C (K x N) = alpha * A^T * B + beta * C_in through the handle's companion engine for A^T.  Strict mode is
bit-identical to cpu_spmm_CSR on CSC_2_CSR(A) (oracle.spmm on the host-transposed CSR), fast mode to the fmaf chain on it."""
import numpy as np
import pytest

from util import ALPHA, BETA, random_csr

pytestmark = pytest.mark.gpu


def oracle_rm(oracle, M, K, rp, ci, v, B, alpha, beta, C0, fma=False):
    """cpu_spmm_CSR (or its fmaf form) on row-major B (K x N) and C (M x N)."""
    N = B.shape[1]
    Cc = np.ascontiguousarray(C0.T).reshape(-1).copy()
    (oracle.spmm_fma if fma else oracle.spmm)(M, N, K, np.float32(alpha), rp, ci, v, np.ascontiguousarray(B.T).reshape(-1),
                                               np.float32(beta), Cc)
    return np.ascontiguousarray(Cc.reshape(N, M).T)


def want_t(oracle, M, K, rp, ci, v, B, alpha, beta, C0, fma=False):
    trp, tci, tv = oracle.csc_to_csr(K, M, np.asarray(rp, np.int32), np.asarray(ci, np.int32), np.asarray(v, np.float32))
    return oracle_rm(oracle, K, M, trp, tci, tv, B, alpha, beta, C0, fma)


def run_t(e, B, alpha, beta, C0, ldb=None, ldc=None, alias=False, b_offset=0):
    """The transposed call on torch buffers with leading dimensions ldb / ldc (padding columns NaN: never read, never written)."""
    import torch
    M, N = B.shape
    K = C0.shape[0]
    ldb, ldc = ldb or N, ldc or N
    dB = torch.full((M * ldb + b_offset,), float("nan"), device="cuda")
    dB[b_offset:].view(M, ldb)[:, :N] = torch.from_numpy(B).cuda()
    dCin = torch.full((K, ldc), float("nan"), device="cuda")
    dCin[:, :N] = torch.from_numpy(C0).cuda()
    dC = dCin if alias else torch.full((K, ldc), -7.0, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    e.spmm_t_device_rm(N, alpha, dB.data_ptr() + 4 * b_offset, ldb, beta, dCin.data_ptr(), ldc, dC.data_ptr(), ldc, st)
    torch.cuda.synchronize()
    out = dC.cpu().numpy()
    if ldc > N and not alias:
        assert (out[:, N:] == -7.0).all(), "padding columns of C_out written"
    return np.ascontiguousarray(out[:, :N])


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("N", [8, 16, 24, 128])
def test_random_matrix_alpha_beta_ld_alias(sx, oracle, N):
    rs = np.random.RandomState(N)
    M, K = 3000, 2000
    rp, ci, v = random_csr(rs, M, K, 9, long_rows=2)
    B = rs.uniform(-1, 1, (M, N)).astype(np.float32); C0 = rs.uniform(-1, 1, (K, N)).astype(np.float32)
    with sx.Engine(0) as e:
        e.set_matrix_csr(M, K, rp, ci, v)
        assert same(run_t(e, B, ALPHA, BETA, C0), want_t(oracle, M, K, rp, ci, v, B, ALPHA, BETA, C0))
        assert e.last_kernel() not in ("", "none")
        got = run_t(e, B, 1.5, 0.0, np.zeros((K, N), np.float32), ldb=N + 8, ldc=N + 4)     # beta = 0, NaN only in unread padding
        assert same(got, want_t(oracle, M, K, rp, ci, v, B, 1.5, 0.0, np.zeros((K, N), np.float32)))
        assert same(run_t(e, B, ALPHA, BETA, C0, ldc=N + 8, alias=True), want_t(oracle, M, K, rp, ci, v, B, ALPHA, BETA, C0))


@pytest.mark.parametrize("matrix", ["fem natural", "fem random order", "kron rectangular", "powerlaw columns"])
def test_structured_matrices(sx, oracle, matrix):
    from sextans_amd import api, holdout, meshgen
    if matrix.startswith("fem"):
        rp, ci, v = api.gen_fem3d_host(24, 22, 20, 3, 7)
        M = K = 24 * 22 * 20 * 3
        if matrix == "fem random order":
            rp, ci, v = meshgen.permute_symmetric(rp, ci, v, M, meshgen.node_permutation(M // 3, 3, 9))
    elif matrix == "kron rectangular":
        rp, ci, v, M, K = holdout.kron_host(6, "rect")
    else:   # long COLUMNS: A^T has hub rows (the exact-chain path of the companion)
        M = K = 40000
        prp, pci, pv = api.gen_powerlaw_host(M, K, 4, 110, 30000, 5)
        rp, ci, v = oracle.csc_to_csr(M, K, prp, pci, pv)
    rs = np.random.RandomState(1)
    N = 16
    B = rs.uniform(-1, 1, (M, N)).astype(np.float32); C0 = rs.uniform(-1, 1, (K, N)).astype(np.float32)
    with sx.Engine(0) as e:
        e.set_matrix_csr(M, K, rp, ci, v)
        assert same(run_t(e, B, ALPHA, BETA, C0), want_t(oracle, M, K, rp, ci, v, B, ALPHA, BETA, C0)), e.last_kernel()
        assert same(run_t(e, B, ALPHA, BETA, C0, b_offset=1), want_t(oracle, M, K, rp, ci, v, B, ALPHA, BETA, C0))   # unaligned B: fallback
        assert e.get_stat("transpose_build_s") > 0


def test_fast_mode_before_and_after_the_transposed_form_exists(sx, oracle):
    rs = np.random.RandomState(2)
    M, K, N = 2500, 3500, 32
    rp, ci, v = random_csr(rs, M, K, 12)
    B = rs.uniform(-1, 1, (M, N)).astype(np.float32); C0 = rs.uniform(-1, 1, (K, N)).astype(np.float32)
    want = want_t(oracle, M, K, rp, ci, v, B, ALPHA, BETA, C0, fma=True)
    with sx.Engine(0) as e:
        e.set_option("mode", 1)
        e.set_matrix_csr(M, K, rp, ci, v)
        assert same(run_t(e, B, ALPHA, BETA, C0), want)
    with sx.Engine(0) as e:
        e.set_matrix_csr(M, K, rp, ci, v)
        assert same(run_t(e, B, ALPHA, BETA, C0), want_t(oracle, M, K, rp, ci, v, B, ALPHA, BETA, C0))
        e.set_option("mode", 1)                       # after the companion exists
        assert same(run_t(e, B, ALPHA, BETA, C0), want)
        e.set_option("mode", 0)
        assert same(run_t(e, B, ALPHA, BETA, C0), want_t(oracle, M, K, rp, ci, v, B, ALPHA, BETA, C0))


def test_new_matrix_drops_the_transposed_form(sx, oracle):
    rs = np.random.RandomState(4)
    N = 16
    with sx.Engine(0) as e:
        for M, K in ((1500, 1000), (900, 1700)):
            rp, ci, v = random_csr(rs, M, K, 7)
            e.set_matrix_csr(M, K, rp, ci, v)
            assert e.get_stat("transpose_build_s") == 0
            B = rs.uniform(-1, 1, (M, N)).astype(np.float32); C0 = rs.uniform(-1, 1, (K, N)).astype(np.float32)
            before = e.get_stat("device_bytes")
            assert same(run_t(e, B, ALPHA, BETA, C0), want_t(oracle, M, K, rp, ci, v, B, ALPHA, BETA, C0))
            assert e.get_stat("device_bytes") >= before + (K + 1) * 4 + len(ci) * 8


def test_prepared_transposed_call_inside_a_graph_capture(sx, oracle):
    import torch
    from sextans_amd import api, meshgen
    rp, ci, v = api.gen_fem3d_host(20, 18, 16, 3, 7)
    M = K = 20 * 18 * 16 * 3
    rp, ci, v = meshgen.permute_symmetric(rp, ci, v, M, meshgen.node_permutation(M // 3, 3, 5))
    N = 32
    rs = np.random.RandomState(6)
    with sx.Engine(0) as e:
        e.set_matrix_csr(M, K, rp, ci, v)
        e.prepare(N, rowmajor=True, transposed=True)
        build_s = e.get_stat("transpose_build_s")
        assert build_s > 0
        dB = torch.empty((M, N), device="cuda"); dCin = torch.empty((K, N), device="cuda"); dC = torch.empty((K, N), device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            st = torch.cuda.current_stream().cuda_stream
            e.spmm_t_device_rm(N, ALPHA, dB.data_ptr(), N, BETA, dCin.data_ptr(), N, dC.data_ptr(), N, st)
        assert e.get_stat("transpose_build_s") == build_s
        for trial in range(2):
            B = rs.uniform(-1, 1, (M, N)).astype(np.float32); C0 = rs.uniform(-1, 1, (K, N)).astype(np.float32)
            dB.copy_(torch.from_numpy(B)); dCin.copy_(torch.from_numpy(C0))
            g.replay()
            torch.cuda.synchronize()
            assert same(dC.cpu().numpy(), want_t(oracle, M, K, rp, ci, v, B, ALPHA, BETA, C0)), (trial, e.last_kernel())
