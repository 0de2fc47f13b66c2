"""torch op backward: spmm(A, B, alpha, beta, C) is an autograd node when A (its values), B or C requires grad.  dB = alpha * A^T G on the
transposed entry, dA = alpha * (G B^T) on A's pattern by the SDDMM kernel, dC = beta * G -- bit-identical to the oracle / the SDDMM
restatement, and within the fast-mode tolerance of dense torch autograd."""
import numpy as np
import pytest

from test_sddmm_gpu import sddmm_ref
from test_spmm_transposed_gpu import oracle_rm, want_t
from util import random_csr

pytestmark = pytest.mark.gpu

ALPHA, BETA = 0.85, -2.06


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def make_A(rp, ci, v, M, K, leaf):
    """(A, the tensor whose .grad receives dA): a leaf CSR tensor, or a CSR tensor built from a values tensor that requires grad."""
    import torch
    crow = torch.from_numpy(rp.astype(np.int64)).cuda(); col = torch.from_numpy(ci.astype(np.int64)).cuda()
    val = torch.from_numpy(v).cuda()
    if leaf:
        A = torch.sparse_csr_tensor(crow, col, val, size=(M, K)).requires_grad_()
        return A, A
    val.requires_grad_()
    return torch.sparse_csr_tensor(crow, col, val, size=(M, K)), val


def grad_values(holder):
    g = holder.grad
    return (g.values() if g.layout == __import__("torch").sparse_csr else g).detach().cpu().numpy()


@pytest.mark.parametrize("N", [20, 128])
@pytest.mark.parametrize("leaf", [True, False])
@pytest.mark.parametrize("with_c", [False, True])
@pytest.mark.parametrize("transpose_a", [False, True])
def test_exact_gradients(sx, oracle, N, leaf, with_c, transpose_a):
    import torch
    from sextans_amd import torch_op
    rs = np.random.RandomState(N + 2 * leaf + 4 * with_c)
    M, K = 900, 700
    rp, ci, v = random_csr(rs, M, K, 8)
    A, holder = make_A(rp, ci, v, M, K, leaf)
    rows_b, rows_c = (M, K) if transpose_a else (K, M)
    Bn = rs.uniform(-1, 1, (rows_b, N)).astype(np.float32)
    Cn = rs.uniform(-1, 1, (rows_c, N)).astype(np.float32)
    Gn = rs.uniform(-1, 1, (rows_c, N)).astype(np.float32)
    B = torch.from_numpy(Bn).cuda().requires_grad_()
    C = torch.from_numpy(Cn).cuda().requires_grad_() if with_c else None
    beta = BETA if with_c else 0.0
    out = torch_op.spmm(A, B, ALPHA, beta, C, transpose_a=transpose_a)
    assert out.grad_fn is not None
    out.backward(torch.from_numpy(Gn).cuda())
    if transpose_a:
        want_b = oracle_rm(oracle, M, K, rp, ci, v, Gn, ALPHA, 0.0, np.zeros((M, N), np.float32))
        want_a = sddmm_ref(rp, ci, Bn, Gn, ALPHA)
    else:
        want_b = want_t(oracle, M, K, rp, ci, v, Gn, ALPHA, 0.0, np.zeros((K, N), np.float32))
        want_a = sddmm_ref(rp, ci, Gn, Bn, ALPHA)
    assert same(B.grad.cpu().numpy(), want_b)
    assert holder.grad is not None and same(grad_values(holder), want_a)
    if leaf:
        assert A.grad.layout == torch.sparse_csr and A.grad.crow_indices().dtype == torch.int64
        assert torch.equal(A.grad.col_indices(), A.col_indices())
    if with_c:
        assert np.allclose(C.grad.cpu().numpy(), np.float32(BETA) * Gn, rtol=1e-6, atol=0)
    torch_op.clear_cache()


def _close(got, want, rtol=2e-4):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.all(np.abs(got - want) <= rtol * (np.abs(want) + np.abs(want).max() * 1e-2))


@pytest.mark.parametrize("fast", [False, True])
def test_against_dense_autograd_two_layers(sx, fast):
    import torch
    from sextans_amd import torch_op
    rs = np.random.RandomState(11)
    M = K = 1200
    rp, ci, v = random_csr(rs, M, K, 10)
    A, val = make_A(rp, ci, v, M, K, leaf=False)
    X = torch.from_numpy(rs.uniform(-1, 1, (K, 24)).astype(np.float32)).cuda().requires_grad_()
    W = torch.from_numpy(rs.uniform(-1, 1, (24, 16)).astype(np.float32)).cuda().requires_grad_()
    R = torch.from_numpy(rs.uniform(-1, 1, (M, 16)).astype(np.float32)).cuda()
    Z = torch_op.spmm(A, torch_op.spmm(A, X, fast=fast) @ W, 0.5, fast=fast)
    (Z * R).sum().backward()
    Ad = torch.zeros((M, K), device="cuda")
    rows = torch.from_numpy(np.repeat(np.arange(M), np.diff(rp))).cuda()
    Ad[rows, torch.from_numpy(ci.astype(np.int64)).cuda()] = torch.from_numpy(v).cuda()
    Ad.requires_grad_()
    Xd = X.detach().clone().requires_grad_(); Wd = W.detach().clone().requires_grad_()
    Zd = 0.5 * (Ad @ ((Ad @ Xd) @ Wd))
    (Zd * R).sum().backward()
    assert _close(X.grad.cpu().numpy(), Xd.grad.cpu().numpy())
    assert _close(W.grad.cpu().numpy(), Wd.grad.cpu().numpy())
    assert _close(val.grad.cpu().numpy(), Ad.grad[rows, torch.from_numpy(ci.astype(np.int64)).cuda()].cpu().numpy())
    torch_op.clear_cache()


def test_errors_and_no_grad_path(sx, oracle):
    import torch
    from sextans_amd import torch_op
    rs = np.random.RandomState(7)
    M, K, N = 600, 500, 16
    rp, ci, v = random_csr(rs, M, K, 6)
    A, val = make_A(rp, ci, v, M, K, leaf=False)
    B = torch.from_numpy(rs.uniform(-1, 1, (K, N)).astype(np.float32)).cuda().requires_grad_()
    with pytest.raises(RuntimeError):
        torch_op.spmm(A, B, out=torch.empty((M, N), device="cuda"))
    out = torch_op.spmm(A, B)
    with torch.no_grad():
        val.mul_(2.0)
    with pytest.raises(RuntimeError):
        out.sum().backward()
    A2, _ = make_A(rp, ci, v, M, K, leaf=True)
    with torch.no_grad():
        got = torch_op.spmm(A2, B, ALPHA)
    assert got.grad_fn is None
    want = oracle_rm(oracle, M, K, rp, ci, v, B.detach().cpu().numpy(), ALPHA, 0.0, np.zeros((M, N), np.float32))
    assert same(got.cpu().numpy(), want)
    torch_op.clear_cache()


def test_captured_training_step(sx, oracle):
    import torch
    from sextans_amd import api, meshgen, torch_op
    rp, ci, v = api.gen_fem3d_host(16, 15, 14, 3, 7)
    M = K = 16 * 15 * 14 * 3
    rp, ci, v = meshgen.permute_symmetric(rp, ci, v, M, meshgen.node_permutation(M // 3, 3, 2))
    N = 16
    rs = np.random.RandomState(8)
    A, _ = make_A(rp, ci, v, M, K, leaf=True)
    B = torch.from_numpy(rs.uniform(-1, 1, (K, N)).astype(np.float32)).cuda().requires_grad_()
    G = torch.from_numpy(rs.uniform(-1, 1, (M, N)).astype(np.float32)).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                      # warm-up step: engine, A^T, plans
        torch_op.spmm(A, B, ALPHA).backward(G)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    A.grad = None; B.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        torch_op.spmm(A, B, ALPHA).backward(G)
    for trial in range(2):
        Bn = rs.uniform(-1, 1, (K, N)).astype(np.float32)
        with torch.no_grad():
            B.copy_(torch.from_numpy(Bn))
        g.replay()
        torch.cuda.synchronize()
        Gn = G.cpu().numpy()
        assert same(B.grad.cpu().numpy(), want_t(oracle, M, K, rp, ci, v, Gn, ALPHA, 0.0, np.zeros((K, N), np.float32))), trial
        assert same(A.grad.values().cpu().numpy(), sddmm_ref(rp, ci, Gn, Bn, ALPHA)), trial
    torch_op.clear_cache()
