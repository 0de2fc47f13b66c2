"""torch ops for attention over a fixed sparsity pattern: sddmm (the bits of the SDDMM restatement), row_softmax and sparse_attention
(against a dense float64 masked-softmax attention and its autograd, with the tolerance test_torch_autograd_gpu.py uses for chains of fp32
ops), one cached engine for the whole pipeline, and a captured training step."""
import numpy as np
import pytest

from test_sddmm_gpu import sddmm_ref
from test_torch_autograd_gpu import _close
from util import random_csr

pytestmark = pytest.mark.gpu

LR = 0.05


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def pattern(seed, M, K, mean):
    """random pattern without empty rows (a dense masked softmax has no answer for a row without entries)"""
    rs = np.random.RandomState(seed)
    rp, ci, v = random_csr(rs, M, K, mean, empty_frac=0.0)
    lens = np.diff(rp)
    if np.any(lens == 0):
        rp2 = np.zeros(M + 1, np.int32); rp2[1:] = np.cumsum(np.maximum(lens, 1))
        ci2 = np.zeros(rp2[-1], np.int32)
        for r in range(M):
            ci2[rp2[r]:rp2[r + 1]] = ci[rp[r]:rp[r + 1]] if lens[r] else [r % K]
        rp, ci = rp2, ci2
        v = rs.uniform(-1, 1, len(ci)).astype(np.float32)
    return rs, rp, ci, v


def make_A(rp, ci, v, M, K, grad=False, dtype=np.int64):
    import torch
    crow, col = torch.from_numpy(rp.astype(dtype)).cuda(), torch.from_numpy(ci.astype(dtype)).cuda()
    A = torch.sparse_csr_tensor(crow, col, torch.from_numpy(v).cuda(), size=(M, K))
    return A.requires_grad_() if grad else A


def test_sddmm_has_the_bits_of_the_restatement(sx):
    import torch
    from sextans_amd import torch_op
    rs = np.random.RandomState(3)
    M, K = 1100, 900
    rp, ci, v = random_csr(rs, M, K, 9, empty_frac=0.1, long_rows=1)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    for N in (16, 20, 64):
        Xn = rs.uniform(-1, 1, (M, N)).astype(np.float32); Yn = rs.uniform(-1, 1, (K, N)).astype(np.float32)
        X, Y = torch.from_numpy(Xn).cuda(), torch.from_numpy(Yn).cuda()
        S = torch_op.sddmm(A, X, Y, 0.85)
        assert S.layout == torch.sparse_csr and S.values().dtype == torch.float32 and tuple(S.shape) == (M, K)
        assert same(S.values().cpu().numpy(), sddmm_ref(rp, ci, Xn, Yn, 0.85)), N
        S = torch_op.sddmm(A, X, Y, 0.85, beta=1.0)
        assert same(S.values().cpu().numpy(), sddmm_ref(rp, ci, Xn, Yn, 0.85, 1.0, v)), N
        assert S.crow_indices().data_ptr() == A.crow_indices().data_ptr() and S.col_indices().data_ptr() == A.col_indices().data_ptr()
    assert torch_op.cache_info()["engines_built"] == 1
    torch_op.clear_cache()


def dense_attention(rp, ci, v, M, K, Qn, Kn, Vn, scale, bias):
    """float64 masked-softmax attention on the pattern: (out, leaves Q, K, V, Avals) for autograd"""
    import torch
    rows = torch.from_numpy(np.repeat(np.arange(M), np.diff(rp))).cuda()
    cols = torch.from_numpy(ci.astype(np.int64)).cuda()
    Q, Kt, V = (torch.from_numpy(t).cuda().double().requires_grad_() for t in (Qn, Kn, Vn))
    Av = torch.from_numpy(v).cuda().double().requires_grad_()
    mask = torch.full((M, K), float("-inf"), dtype=torch.float64, device="cuda")
    mask[rows, cols] = 0.0
    Ad = torch.zeros((M, K), dtype=torch.float64, device="cuda").index_put((rows, cols), Av)
    S = Q @ Kt.T + (Ad if bias else 0.0)
    P = torch.softmax(S * scale + mask, dim=1)
    return P @ V, P, (Q, Kt, V, Av), (rows, cols)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("d, dv", [(16, 16), (20, 40)])
def test_sparse_attention_against_dense_float64(sx, bias, d, dv):
    import torch
    from sextans_amd import torch_op
    M, K = 700, 600
    rs, rp, ci, v = pattern(11 + d, M, K, 9)
    Qn, Kn = rs.uniform(-1, 1, (M, d)).astype(np.float32), rs.uniform(-1, 1, (K, d)).astype(np.float32)
    Vn = rs.uniform(-1, 1, (K, dv)).astype(np.float32)
    Gn = rs.uniform(-1, 1, (M, dv)).astype(np.float32)
    scale = None if d == 16 else 0.37
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K, grad=bias)
    Q, Kt, V = (torch.from_numpy(t).cuda().requires_grad_() for t in (Qn, Kn, Vn))
    out = torch_op.sparse_attention(A, Q, Kt, V, scale=scale, bias=bias)
    out.backward(torch.from_numpy(Gn).cuda())
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] > 0, info
    want, _, (Qd, Kd, Vd, Avd), _ = dense_attention(rp, ci, v, M, K, Qn, Kn, Vn, 1.0 / np.sqrt(d) if scale is None else scale, bias)
    want.backward(torch.from_numpy(Gn).cuda().double())
    assert _close(out.detach().cpu().numpy(), want.detach().cpu().numpy())
    assert _close(Q.grad.cpu().numpy(), Qd.grad.cpu().numpy())
    assert _close(Kt.grad.cpu().numpy(), Kd.grad.cpu().numpy())
    assert _close(V.grad.cpu().numpy(), Vd.grad.cpu().numpy())
    if bias:
        assert A.grad.layout == torch.sparse_csr
        assert _close(A.grad.values().cpu().numpy(), Avd.grad.cpu().numpy())
    else:
        assert A.grad is None
    torch_op.clear_cache()


def test_row_softmax_op_and_shared_index_tensors(sx):
    import torch
    from sextans_amd import torch_op
    M, K = 500, 400
    rs, rp, ci, v = pattern(5, M, K, 7)
    torch_op.clear_cache()
    crow, col = torch.from_numpy(rp.astype(np.int64)).cuda(), torch.from_numpy(ci.astype(np.int64)).cuda()
    val = torch.from_numpy((v * 4).astype(np.float32)).cuda().requires_grad_()
    S = torch.sparse_csr_tensor(crow, col, val, size=(M, K))
    P = torch_op.row_softmax(S, scale=1.7)
    assert P.layout == torch.sparse_csr and P.values().dtype == torch.float32
    assert P.crow_indices().data_ptr() == crow.data_ptr() and P.col_indices().data_ptr() == col.data_ptr()
    Gn = rs.uniform(-1, 1, len(ci)).astype(np.float32)
    P.backward(torch.sparse_csr_tensor(crow, col, torch.from_numpy(Gn).cuda(), size=(M, K)))
    # dense float64 reference
    rows = torch.from_numpy(np.repeat(np.arange(M), np.diff(rp))).cuda()
    vd = torch.from_numpy((v * 4).astype(np.float32)).cuda().double().requires_grad_()
    dense = torch.full((M, K), float("-inf"), dtype=torch.float64, device="cuda").index_put((rows, col), vd * 1.7)
    Pd = torch.softmax(dense, dim=1)[rows, col]
    Pd.backward(torch.from_numpy(Gn).cuda().double())
    assert _close(P.values().detach().cpu().numpy(), Pd.detach().cpu().numpy())
    assert _close(val.grad.cpu().numpy(), vd.grad.cpu().numpy())
    # float64 values are converted as spmm converts them, and come back in their dtype
    P64 = torch_op.row_softmax(torch.sparse_csr_tensor(crow, col, val.detach().double(), size=(M, K)), scale=1.7)
    assert P64.values().dtype == torch.float64 and same(P64.values().float().cpu().numpy(), P.values().detach().cpu().numpy())
    # the pipeline's intermediate results carry A's own index tensors
    A = torch.sparse_csr_tensor(crow, col, torch.from_numpy(v).cuda(), size=(M, K))
    X = torch.from_numpy(rs.uniform(-1, 1, (M, 16)).astype(np.float32)).cuda()
    Y = torch.from_numpy(rs.uniform(-1, 1, (K, 16)).astype(np.float32)).cuda()
    P2 = torch_op.row_softmax(torch_op.sddmm(A, X, Y))
    for T in (P2,):
        assert T.crow_indices().data_ptr() == A.crow_indices().data_ptr() and T.col_indices().data_ptr() == A.col_indices().data_ptr()
    assert torch_op.cache_info()["engines_built"] == 1
    torch_op.clear_cache()


def test_captured_attention_training_step(sx):
    """forward, backward and an SGD update of Q, K and V in place, captured once (refresh(A) outside the capture first) and replayed three
    times: bit for bit three eager steps.  With bias=True A's values enter the scores; they were updated in place before, so the version
    counters A's index tensors share with them have moved -- the pipeline must not answer that with a read-back on every call."""
    import torch
    from sextans_amd import torch_op
    M, K, d = 900, 900, 16
    rs, rp, ci, v = pattern(21, M, K, 10)
    Qn, Kn, Vn = (rs.uniform(-1, 1, (n, d)).astype(np.float32) for n in (M, K, K))
    G = torch.from_numpy(rs.uniform(-1, 1, (M, d)).astype(np.float32)).cuda()

    def start():
        A = make_A(rp, ci, v, M, K)
        with torch.no_grad():
            A.values().mul_(0.5)          # (in place: moves the version counter of A's index tensors too)
        return A, [torch.from_numpy(t).cuda().requires_grad_() for t in (Qn, Kn, Vn)]

    def step(A, params):
        for t in params:
            t.grad = None
        out = torch_op.sparse_attention(A, *params, bias=True)
        out.backward(G)
        with torch.no_grad():
            for t in params:
                t.sub_(LR * t.grad)
        return out

    def state(out, params):
        return [out.detach().cpu().numpy().copy()] + [t.detach().cpu().numpy().copy() for t in params]

    torch_op.clear_cache()
    A, params = start()
    eager = [state(step(A, params), params) for _ in range(4)]
    assert not np.array_equal(eager[3][1], eager[0][1])
    torch_op.clear_cache()
    A, params = start()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(A, params)                   # warm-up: engine, A^T, plans, softmax tables
        torch_op.refresh(A)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step(A, params)
    assert torch_op.cache_info()["engines_built"] == 1
    for k in range(1, 4):
        g.replay()
        torch.cuda.synchronize()
        got = state(out, params)
        for i in range(4):
            assert same(got[i], eager[k][i]), (k, i)
    torch_op.clear_cache()


def test_errors(sx):
    import torch
    from sextans_amd import torch_op
    M, K = 60, 50
    rs, rp, ci, v = pattern(2, M, K, 4)
    A = make_A(rp, ci, v, M, K)
    Q, Kt, V = torch.zeros(M, 16, device="cuda"), torch.zeros(K, 16, device="cuda"), torch.zeros(K, 8, device="cuda")
    with pytest.raises(TypeError):
        torch_op.sddmm(A.to_dense(), Q, Kt)
    with pytest.raises(TypeError):
        torch_op.sddmm(A.cpu(), Q, Kt)
    with pytest.raises(TypeError):
        torch_op.sddmm(A, Q.cpu(), Kt)
    with pytest.raises(TypeError):
        torch_op.row_softmax(A.to_dense())
    with pytest.raises(TypeError):
        torch_op.sparse_attention(A.to_dense(), Q, Kt, V)
    with pytest.raises(TypeError):
        torch_op.sparse_attention(A, Q, Kt, V.cpu())
    with pytest.raises(ValueError):
        torch_op.sddmm(A, Q[:-1], Kt)
    with pytest.raises(ValueError):
        torch_op.sddmm(A, Q, Kt[:, :8])
    with pytest.raises(ValueError):
        torch_op.sparse_attention(A, Q, Kt, V[:-1])
    with pytest.raises(ValueError):
        torch_op.sparse_attention(A, Q, Kt[:-1], V)
    torch_op.clear_cache()
