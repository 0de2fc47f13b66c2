"""sextans_amd.vector_attention.vector_attention on the GPU: forward and the gradients of S, V and D against a float64 torch composition
(a dense masked softmax per channel) on a 60 x 50 random pattern with empty rows, N = 5 (no multiple of 8: the padded copies) and
N = 16; trailing shapes and non-contiguous operands; only the gradients asked for; return_lse; one cached engine and no value refresh;
misuse.  Tolerance: test_torch_autograd_gpu._close (rtol 2e-4); the rows here have about 6 entries, far fewer than those of
test_vector_attention_gpu.py, whose emulation stays below 0.08 of that limit."""
import numpy as np
import pytest

from test_fused_attention_gpu import rand, same
from test_spmm_edge_softagg_gpu import limit_ratio, rows_of
from test_spmm_softagg_gpu import lse_close
from test_torch_attention_gpu import make_A
from test_torch_autograd_gpu import _close
from test_vector_attention_gpu import MODES
from util import random_csr

pytestmark = pytest.mark.gpu

M, K = 60, 50
_cases = {}


def case(N):
    """the pattern (empty rows among its 60) with S in +-4, V, D and G in +-1, once per N"""
    if N not in _cases:
        rs = np.random.RandomState(60)
        rp, ci, v = random_csr(rs, M, K, 6, empty_frac=0.15)
        assert 3 <= np.count_nonzero(np.diff(rp) == 0) < M // 2
        nnz = len(ci)
        _cases[N] = (rp, ci, v, rand(rs, nnz, N) * np.float32(4), rand(rs, K, N), rand(rs, nnz, N), rand(rs, M, N))
    return _cases[N]


def dense_reference(mode, rp, ci, S, V, D, G):
    """float64 on the CPU with torch's autograd, a dense masked softmax over the K columns per (row, channel): (C, lse, dS, dV, dD),
    None for the operand the mode does not have"""
    import torch
    N = S.shape[1]
    rows, cols = torch.from_numpy(rows_of(rp)), torch.from_numpy(ci.astype(np.int64))
    St = torch.from_numpy(S.astype(np.float64)).requires_grad_()
    Vt = torch.from_numpy(V.astype(np.float64)).requires_grad_() if mode != "edge" else None
    Dt = torch.from_numpy(D.astype(np.float64)).requires_grad_() if mode != "node" else None
    sd = torch.full((M, K, N), -np.inf, dtype=torch.float64).index_put((rows, cols), St)
    present = torch.zeros((M, K, 1), dtype=torch.bool).index_put((rows, cols), torch.ones((len(ci), 1), dtype=torch.bool))
    msg = torch.zeros((M, K, N), dtype=torch.float64)
    if Dt is not None:
        msg = msg.index_put((rows, cols), Dt)
    if Vt is not None:
        msg = msg + Vt[None]
    mx = sd.detach().amax(1, keepdim=True)
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))   # an empty row: every weight is 0
    w = torch.where(present, torch.exp(sd - mx), torch.zeros_like(sd))
    z = w.sum(1)
    C = (w * msg).sum(1) / torch.where(z > 0, z, torch.ones_like(z))
    lse = torch.where(z > 0, mx[:, 0] + torch.log(z), torch.full_like(z, -np.inf))
    C.backward(torch.from_numpy(G.astype(np.float64)))
    g = lambda t: t.grad.numpy() if t is not None else None   # noqa: E731
    return C.detach().numpy(), lse.detach().numpy(), g(St), g(Vt), g(Dt)


def operands(mode, S, V, D, grad=True):
    import torch
    t = lambda x: torch.from_numpy(x).cuda().requires_grad_(grad)   # noqa: E731
    return t(S), (t(V) if mode != "edge" else None), (t(D) if mode != "node" else None)


@pytest.mark.parametrize("N", [5, 16])
@pytest.mark.parametrize("mode", list(MODES))
def test_forward_and_gradients(sx, mode, N):
    import torch
    from sextans_amd import torch_op
    from sextans_amd.vector_attention import vector_attention
    rp, ci, v, S, V, D, G = case(N)
    want = dense_reference(mode, rp, ci, S, V, D, G)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    St, Vt, Dt = operands(mode, S, V, D)
    out, lse = vector_attention(A, St, Vt, Dt, return_lse=True)
    assert out.requires_grad and not lse.requires_grad and out.shape == (M, N) and lse.shape == (M, N)
    out.backward(torch.from_numpy(G).cuda())
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0 and info["entries"] == 1, info
    got = (out.detach(), lse, St.grad, Vt.grad if Vt is not None else None, Dt.grad if Dt is not None else None)
    for name, g, w in zip(("C", "lse", "dS", "dV", "dD"), got, want):
        assert (g is None) == (w is None), name
        if w is None:
            continue
        g = g.cpu().numpy()
        assert g.shape == w.shape, name
        print(mode, N, name, "error / limit", limit_ratio(g, w))
        assert lse_close(g, w) if name == "lse" else _close(g, w), name
    empty = np.diff(rp) == 0
    assert np.all(got[0].cpu().numpy()[empty] == 0) and np.all(St.grad.cpu().numpy() * 0 == 0)
    # without autograd: the same bits, with and without lse
    with torch.no_grad():
        assert same(vector_attention(A, St, Vt, Dt).cpu().numpy(), out.detach().cpu().numpy())
        o2, l2 = vector_attention(A, St, Vt, Dt, return_lse=True)
        assert same(o2.cpu().numpy(), out.detach().cpu().numpy()) and same(l2.cpu().numpy(), lse.cpu().numpy())
    # .sum().backward(): an upstream gradient with zero strides
    St.grad = None
    vector_attention(A, St, Vt, Dt).sum().backward()
    ones = dense_reference(mode, rp, ci, S, V, D, np.ones((M, N), np.float32))
    assert _close(St.grad.cpu().numpy(), ones[2])
    assert torch_op.cache_info() == info
    torch_op.clear_cache()


def test_trailing_shapes_and_non_contiguous_operands(sx):
    """operands with a (., 2, 8) trailing shape; column slices of wider tensors and a transposed V; a -inf score masks its entry"""
    import torch
    from sextans_amd import torch_op
    from sextans_amd.vector_attention import vector_attention
    N = 16
    rp, ci, v, S, V, D, G = case(N)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    St, Vt, Dt = operands("add", S, V, D)
    flat = vector_attention(A, St, Vt, Dt)
    flat.backward(torch.from_numpy(G).cuda())
    S3, V3, D3 = (x.detach().reshape(-1, 2, 8).requires_grad_() for x in (St, Vt, Dt))
    out, lse = vector_attention(A, S3, V3, D3, return_lse=True)
    assert out.shape == (M, 2, 8) and lse.shape == (M, 2, 8)
    out.backward(torch.from_numpy(G).cuda().reshape(M, 2, 8))
    assert same(out.detach().reshape(M, N).cpu().numpy(), flat.detach().cpu().numpy())
    for x3, x in ((S3, St), (V3, Vt), (D3, Dt)):
        assert x3.grad.shape == x3.shape and same(x3.grad.reshape(-1, N).cpu().numpy(), x.grad.cpu().numpy())
    # non-contiguous: every second column of a wider S, a transposed V, a D with a row stride the kernel cannot read (N + 1)
    Sw = torch.zeros((len(ci), 2 * N), device="cuda")
    Sw[:, ::2] = St.detach()
    Vw = Vt.detach().t().contiguous().t()
    Dw = torch.zeros((len(ci), N + 1), device="cuda")
    Dw[:, :N] = Dt.detach()
    Sn, Vn, Dn = Sw[:, ::2].requires_grad_(), Vw.requires_grad_(), Dw[:, :N].requires_grad_()
    assert not Sn.is_contiguous() and not Vn.is_contiguous() and not Dn.is_contiguous()
    out = vector_attention(A, Sn, Vn, Dn)
    out.backward(torch.from_numpy(G).cuda())
    assert same(out.detach().cpu().numpy(), flat.detach().cpu().numpy())
    for xn, x in ((Sn, St), (Vn, Vt), (Dn, Dt)):
        assert same(xn.grad.cpu().numpy(), x.grad.cpu().numpy())
    # a masked entry: the result of the pattern's other entries, gradient 0
    r0 = int(np.flatnonzero(np.diff(rp) > 2)[0])
    S2 = S.copy()
    S2[rp[r0]] = -np.inf
    want = dense_reference("add", rp, ci, S2, V, D, G)
    Sm = torch.from_numpy(S2).cuda().requires_grad_()
    out = vector_attention(A, Sm, Vt.detach(), Dt.detach())
    out.backward(torch.from_numpy(G).cuda())
    assert _close(out.detach().cpu().numpy(), want[0]) and _close(Sm.grad.cpu().numpy(), want[2])
    assert np.all(Sm.grad[rp[r0]].cpu().numpy().view(np.uint32) == 0)
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0 and info["entries"] == 1, info
    torch_op.clear_cache()


@pytest.mark.parametrize("mode", list(MODES))
def test_only_the_gradients_asked_for(sx, mode):
    """each requires_grad subset returns only what is asked, with the bits of the full call"""
    import itertools
    import torch
    from sextans_amd import torch_op
    from sextans_amd.vector_attention import vector_attention
    N = 16
    rp, ci, v, S, V, D, G = case(N)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    Gt = torch.from_numpy(G).cuda()
    full = operands(mode, S, V, D)
    vector_attention(A, *full).backward(Gt)
    have = [i for i, x in enumerate(full) if x is not None]
    for k in range(len(have) + 1):
        for subset in itertools.combinations(have, k):
            ops = [None if x is None else x.detach().clone().requires_grad_(i in subset) for i, x in enumerate(full)]
            out = vector_attention(A, *ops)
            assert out.requires_grad == bool(subset)
            if subset:
                out.backward(Gt)
            for i, x in enumerate(ops):
                if x is None:
                    continue
                if i in subset:
                    assert same(x.grad.cpu().numpy(), full[i].grad.cpu().numpy()), (subset, i)
                else:
                    assert x.grad is None, (subset, i)
    # A gets no gradient even when it asks
    Ag = make_A(rp, ci, v, M, K, grad=True)
    vector_attention(Ag, *[None if x is None else x.detach().requires_grad_() for x in full]).backward(Gt)
    assert Ag.grad is None
    # not twice differentiable
    ops = [None if x is None else x.detach().requires_grad_() for x in full]
    g, = torch.autograd.grad(vector_attention(A, *ops), ops[0], Gt, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    torch_op.clear_cache()


def test_misuse(sx):
    import torch
    from sextans_amd import torch_op
    from sextans_amd.vector_attention import vector_attention as f
    N = 16
    rp, ci, v, S, V, D, G = case(N)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    St, Vt, Dt = operands("add", S, V, D, grad=False)
    with pytest.raises(ValueError):
        f(A, St)                                  # neither V nor D
    with pytest.raises(TypeError):
        f(A, St.cpu(), Vt, Dt)                    # CPU operands
    with pytest.raises(TypeError):
        f(A, St, Vt.cpu())
    with pytest.raises(TypeError):
        f(A, St, None, Dt.cpu())
    with pytest.raises(TypeError):
        f(A.to_dense(), St, Vt)                   # a dense A
    with pytest.raises(TypeError):
        f(A, St, Vt.to_sparse())                  # a sparse operand
    with pytest.raises(ValueError):
        f(A, St[:-1], Vt)                         # shapes
    with pytest.raises(ValueError):
        f(A, St, Vt[:-1])
    with pytest.raises(ValueError):
        f(A, St, None, Dt[:-1])
    with pytest.raises(ValueError):
        f(A, St, Vt[:, :8])
    with pytest.raises(ValueError):
        f(A, St, Vt, Dt.reshape(-1, 2, 8))
    with pytest.raises(ValueError):
        f(A, St[:, 0], Vt[:, 0])                  # 1-D
    with pytest.raises(ValueError):
        f(A, St[:, :0], Vt[:, :0])                # no columns
    assert torch_op.cache_info()["entries"] == 0
    torch_op.clear_cache()
