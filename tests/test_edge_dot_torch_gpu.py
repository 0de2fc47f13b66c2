"""sextans_amd.edge_dot.edge_dot on the GPU: forward and the gradients of x_dst and x_src against the torch composition
(x_dst.double()[rows] * x_src.double()[cols]).sum(-1) (gathers by entry_rows / col_indices, autograd through index_add_) on a 60 x 50
random pattern with empty rows; 2-D and 3-D operands, d = 20 (no multiple of 8: the padded copies), d = 136 (refused), operands the
kernel cannot read in place; x_dst is x_src on a square pattern; only the gradients asked for, the skipped pass shown by last_kernel and
the transpose's build time on a pattern whose long rows are on one side; the chain edge_dot -> score_attention(softmax) against the
fused sparse_attention; misuse.
  Tolerances, derived: an element of S is a chain of d rounded products and d rounded adds of which the first (0 + p) is exact, so to
first order |S - exact| <= (1 + (d - 1)) 2^-24 sum_n |x_n y_n|; one more unit covers the higher-order terms: (d + 1) 2^-24 sum_n
|x_n y_n|.  The gradients: (n + 2) 2^-24 sum |t_e|, the bound of test_edge_op_gpu.py.  The chain: the tolerance of the fused attention
against its composition (test_fused_attention_gpu.test_agrees_with_the_composition: test_torch_autograd_gpu._close)."""
import numpy as np
import pytest

from test_edge_dot_gpu import dot_ref, grad_ref
from test_edge_op_gpu import within_bound
from test_fused_attention_gpu import rand, same
from test_pattern_dealing_gpu import pat
from test_torch_attention_gpu import make_A, pattern
from test_torch_autograd_gpu import _close
from util import random_csr

pytestmark = pytest.mark.gpu

M, K = 60, 50
U = 2.0 ** -24
_cases = {}


def case(H, d):
    """the pattern (empty rows among its 60) with x_dst (M, H, d), x_src (K, H, d) and the upstream gradient (nnz, H) in +-1"""
    if (H, d) not in _cases:
        rs = np.random.RandomState(61)
        rp, ci, v = random_csr(rs, M, K, 6, empty_frac=0.15)
        assert 3 <= np.count_nonzero(np.diff(rp) == 0) < M // 2
        _cases[H, d] = (rp, ci, v, rand(rs, M, H, d), rand(rs, K, H, d), rand(rs, len(ci), H))
    return _cases[H, d]


def compose(A, xd, xs):
    """the torch composition in the operands' dtype: two gathers, one elementwise pass, a sum, autograd through index_add_"""
    from sextans_amd import torch_op
    rows, cols = torch_op.entry_rows(A), A.col_indices().long()
    return (xd[rows] * xs[cols]).sum(-1)


def tensors(*arrays, grad=True, dtype=None):
    import torch
    return [(torch.from_numpy(x).cuda().to(dtype) if dtype else torch.from_numpy(x).cuda()).requires_grad_(grad) for x in arrays]


@pytest.mark.parametrize("H, d, flat", [(1, 16, True), (1, 16, False), (3, 20, False), (2, 8, False), (8, 16, False), (2, 128, False)])
def test_forward_and_gradients(sx, H, d, flat):
    """flat: the operands are (rows, d) and the result (nnz,)"""
    import torch
    from sextans_amd import torch_op
    from sextans_amd.edge_dot import edge_dot
    rp, ci, v, xd, xs, Gs = case(H, d)
    nnz = len(ci)
    if flat:
        xd, xs, Gs = xd[:, 0], xs[:, 0], Gs[:, 0]
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    Gt = torch.from_numpy(Gs).cuda()
    ref = tensors(xd, xs, dtype=torch.float64)
    want = compose(A, *ref)
    want.backward(Gt.double())
    got = tensors(xd, xs)
    out = edge_dot(A, *got)
    assert out.requires_grad and out.shape == ((nnz,) if flat else (nnz, H)) and out.dtype == torch.float32
    out.backward(Gt)
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0 and info["entries"] == 1, info
    # forward: the derived bound against float64; the bits of the sequential float32 loop (zero padding adds +0 at the chain's end)
    with torch.no_grad():
        mag = compose(A, ref[0].abs(), ref[1].abs()).cpu().numpy()
    bound = (d + 1) * U * mag
    err = np.abs(out.detach().cpu().numpy().astype(np.float64) - want.detach().cpu().numpy())
    print(H, d, "forward max err / bound", float((err[bound > 0] / bound[bound > 0]).max()))
    assert np.all(err <= bound)
    loop = dot_ref(rp, ci, xd.reshape(M, H * d), xs.reshape(K, H * d), H, d)
    assert same(out.detach().cpu().numpy().reshape(nnz, H), loop)
    with torch.no_grad():
        assert same(edge_dot(A, *got).cpu().numpy().reshape(nnz, H), loop)   # without autograd: the same bits
    # gradients
    _, mags, counts = grad_ref(rp, ci, xd.reshape(M, H * d), xs.reshape(K, H * d), Gs.reshape(nnz, H), M, K, H, d)
    for name, g, r, n in (("dX", got[0], ref[0], M), ("dY", got[1], ref[1], K)):
        assert g.grad.shape == g.shape and g.grad.dtype == torch.float32
        assert within_bound(g.grad.cpu().numpy().reshape(n, H * d), r.grad.cpu().numpy().reshape(n, H * d), mags[name], counts[name],
                            "%s H=%d d=%d" % (name, H, d)), name
        assert np.all(g.grad.cpu().numpy().reshape(n, H * d)[counts[name] == 0] == 0)
    # .sum().backward(): an upstream gradient with zero strides
    again = tensors(xd, xs)
    edge_dot(A, *again).sum().backward()
    ones = tensors(xd, xs, dtype=torch.float64)
    compose(A, *ones).sum().backward()
    _, mags1, _ = grad_ref(rp, ci, xd.reshape(M, H * d), xs.reshape(K, H * d), np.ones((nnz, H), np.float32), M, K, H, d)
    for name, g, r, n in (("dX", again[0], ones[0], M), ("dY", again[1], ones[1], K)):
        assert within_bound(g.grad.cpu().numpy().reshape(n, H * d), r.grad.cpu().numpy().reshape(n, H * d), mags1[name], counts[name],
                            "sum " + name), name
    assert torch_op.cache_info() == info
    torch_op.clear_cache()


def test_ranks_and_operands_the_kernel_cannot_read_in_place(sx):
    """(rows, d) operands give the bits of (rows, 1, d); rows of a wider tensor are read in place, a transposed operand, a float64 one
    and a column slice at an odd offset are copied: the same bits"""
    import torch
    from sextans_amd import torch_op
    from sextans_amd.edge_dot import edge_dot
    H, d = 2, 8
    rp, ci, v, xd, xs, Gs = case(H, d)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    Gt = torch.from_numpy(Gs).cuda()
    dt, st = tensors(xd, xs)
    whole = edge_dot(A, dt, st)
    whole.backward(Gt)
    # one head at a time through the 2-D call
    for h in range(H):
        d2, s2 = tensors(np.ascontiguousarray(xd[:, h]), np.ascontiguousarray(xs[:, h]))
        one = edge_dot(A, d2, s2)
        assert one.shape == (len(ci),) and same(one.detach().cpu().numpy(), whole.detach()[:, h].cpu().numpy())
        one.backward(Gt[:, h])
        # (the gradient passes deal a row's entries to their lanes by rows x heads: the order of a sum, and so its last bits, may differ
        # with H -- the 2-D gradients are held to the float64 reference in test_forward_and_gradients)
        assert d2.grad.shape == d2.shape and s2.grad.shape == s2.shape
    dw = torch.zeros((M, 2 * H, d), device="cuda")
    dw[:, :H] = dt.detach()
    sw = st.detach().permute(2, 0, 1).contiguous().permute(1, 2, 0)
    dn, sn = dw[:, :H].requires_grad_(), sw.requires_grad_()
    assert not dn.is_contiguous() and not sn.is_contiguous()
    out = edge_dot(A, dn, sn)
    out.backward(Gt.t().contiguous().t())   # a non-contiguous upstream gradient too
    assert same(out.detach().cpu().numpy(), whole.detach().cpu().numpy())
    assert same(dn.grad.cpu().numpy(), dt.grad.cpu().numpy()) and same(sn.grad.cpu().numpy(), st.grad.cpu().numpy())
    odd = torch.zeros((M, H, d + 1), device="cuda")
    odd[:, :, 1:] = dt.detach()
    assert same(edge_dot(A, odd[:, :, 1:], st.detach()).cpu().numpy(), whole.detach().cpu().numpy())
    d64 = dt.detach().double().requires_grad_()
    out = edge_dot(A, d64, st.detach())
    assert out.dtype == torch.float32 and same(out.detach().cpu().numpy(), whole.detach().cpu().numpy())
    out.backward(Gt)
    assert d64.grad.dtype == torch.float64 and same(d64.grad.float().cpu().numpy(), dt.grad.cpu().numpy())
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0 and info["entries"] == 1, info
    torch_op.clear_cache()


def test_x_dst_is_x_src(sx):
    """one tensor for both endpoints of a square pattern: its gradient is the sum of both passes"""
    import torch
    from sextans_amd import torch_op
    from sextans_amd.edge_dot import edge_dot
    H, d, n = 3, 16, 50
    rs = np.random.RandomState(62)
    rp, ci, v = random_csr(rs, n, n, 6, empty_frac=0.15)
    x, Gs = rand(rs, n, H, d), rand(rs, len(ci), H)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, n, n)
    Gt = torch.from_numpy(Gs).cuda()
    xt, = tensors(x)
    out = edge_dot(A, xt, xt)
    out.backward(Gt)
    a, b = tensors(x, x)
    two = edge_dot(A, a, b)
    two.backward(Gt)
    assert same(out.detach().cpu().numpy(), two.detach().cpu().numpy())
    assert same(xt.grad.cpu().numpy(), (a.grad + b.grad).cpu().numpy())
    x64, = tensors(x, dtype=torch.float64)
    compose(A, x64, x64).backward(Gt.double())
    x2 = x.reshape(n, H * d)
    _, mags, counts = grad_ref(rp, ci, x2, x2, Gs, n, n, H, d)
    want = x64.grad.cpu().numpy().reshape(n, H * d)
    bound = ((counts["dX"] + 2)[:, None] * mags["dX"] + (counts["dY"] + 2)[:, None] * mags["dY"]) * U + U * np.abs(want)
    # (both passes' bounds and the rounding of their sum)
    assert np.all(np.abs(xt.grad.cpu().numpy().reshape(n, H * d).astype(np.float64) - want) <= 1.001 * bound)
    with torch.no_grad():
        assert same(edge_dot(A, xt, xt).cpu().numpy(), two.detach().cpu().numpy())
    torch_op.clear_cache()


def test_only_the_gradients_asked_for(sx):
    """each requires_grad subset returns only what is asked, with the bits of the full call; on pattern P (long rows in P, none in P^T)
    last_kernel names the pass that ran: x_dst alone walks P (+long_rows) and builds no A^T, x_src alone walks P^T"""
    import torch
    from sextans_amd import torch_op
    from sextans_amd.edge_dot import edge_dot
    H, d = 3, 8
    p = pat("P")
    rs = np.random.RandomState(63)
    xd, xs, Gs = rand(rs, p.M, H, d), rand(rs, p.K, H, d), rand(rs, p.nnz, H)
    torch_op.clear_cache()
    A = make_A(p.rp, p.ci, np.ones(p.nnz, np.float32), p.M, p.K)
    eng = lambda: list(torch_op._cache.values())[-1].eng   # noqa: E731
    Gt = torch.from_numpy(Gs).cuda()
    t = lambda x, g: torch.from_numpy(x).cuda().requires_grad_(g)   # noqa: E731
    ops = [t(xd, False), t(xs, False)]
    out = edge_dot(A, *ops)
    assert not out.requires_grad and eng().last_kernel() == "edge_dot"
    ops = [t(xd, True), t(xs, False)]
    edge_dot(A, *ops).backward(Gt)
    assert eng().last_kernel() == "edge_dot_backward+long_rows" and eng().get_stat("transpose_build_s") == 0
    assert ops[1].grad is None
    dx_alone = ops[0].grad
    ops = [t(xd, False), t(xs, True)]
    edge_dot(A, *ops).backward(Gt)
    assert eng().last_kernel() == "edge_dot_backward" and eng().get_stat("transpose_build_s") > 0
    assert ops[0].grad is None
    dy_alone = ops[1].grad
    full = [t(xd, True), t(xs, True)]
    edge_dot(A, *full).backward(Gt)
    assert eng().last_kernel() == "edge_dot_backward+long_rows"
    assert same(full[0].grad.cpu().numpy(), dx_alone.cpu().numpy()) and same(full[1].grad.cpu().numpy(), dy_alone.cpu().numpy())
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0 and info["entries"] == 1, info
    # A gets no gradient even when it asks
    Ag = make_A(p.rp, p.ci, np.ones(p.nnz, np.float32), p.M, p.K, grad=True)
    edge_dot(Ag, *[x.detach().requires_grad_() for x in full]).backward(Gt)
    assert Ag.grad is None
    # not twice differentiable
    ops = [x.detach().requires_grad_() for x in full]
    g, = torch.autograd.grad(edge_dot(A, *ops), ops[0], Gt, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    torch_op.clear_cache()


def test_chain_into_score_attention_against_the_fused_attention(sx):
    """edge_dot -> score_attention(normalize="softmax") is sparse_attention(fused=True) on the same Q * scale, K, V, within the
    tolerance the fused attention is held to against its own composition"""
    import torch
    from sextans_amd import torch_op
    from sextans_amd.edge_dot import edge_dot
    Mq, Kk, H, d, dv = 500, 420, 3, 16, 32
    rs, rp, ci, v = pattern(41, Mq, Kk, 11)
    scale = np.float32(1.0 / np.sqrt(d))
    Qn, Kn, Vn, Gn = rand(rs, Mq, H, d) * scale, rand(rs, Kk, H, d), rand(rs, Kk, H, dv), rand(rs, Mq, H, dv)
    assert Qn.dtype == np.float32
    torch_op.clear_cache()
    A = make_A(rp, ci, v, Mq, Kk)
    G = torch.from_numpy(Gn).cuda()
    chain = tensors(Qn, Kn, Vn)
    S = edge_dot(A, chain[0], chain[1])
    torch_op.score_attention(A, S, chain[2], normalize="softmax").backward(G)
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0 and info["entries"] == 1, info
    fused = tensors(Qn, Kn, Vn)
    O = torch_op.sparse_attention(A, *fused, scale=1.0, fused=True)
    O.backward(G)
    with torch.no_grad():
        Oc = torch_op.score_attention(A, S.detach(), chain[2].detach(), normalize="softmax")
    assert _close(Oc.cpu().numpy(), O.detach().cpu().numpy()), "O"
    for c, f, name in zip(chain, fused, ("dQ", "dK", "dV")):
        print(name, "max |chain - fused|", float((c.grad - f.grad).abs().max()), "max |fused|", float(f.grad.abs().max()))
        assert _close(c.grad.cpu().numpy(), f.grad.cpu().numpy()), name
    torch_op.clear_cache()


def test_misuse(sx):
    import torch
    from sextans_amd import torch_op
    from sextans_amd.edge_dot import edge_dot as f
    H, d = 2, 8
    rp, ci, v, xd, xs, Gs = case(H, d)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    dt, st = tensors(xd, xs, grad=False)
    z = lambda *shape: torch.zeros(shape, device="cuda")   # noqa: E731
    with pytest.raises(ValueError, match="d up to 128"):
        f(A, z(M, 1, 136), z(K, 1, 136))              # d beyond the kernels' head dimension
    with pytest.raises(ValueError, match="d up to 128"):
        f(A, z(M, 136), z(K, 136))
    with pytest.raises(TypeError):
        f(A, dt.cpu(), st)                            # CPU operands
    with pytest.raises(TypeError):
        f(A, dt, st.cpu())
    with pytest.raises(TypeError):
        f(A.to_dense(), dt, st)                       # a dense A
    with pytest.raises(TypeError):
        f(A, dt, st.to_sparse())                      # a sparse operand
    with pytest.raises(ValueError):
        f(A, dt[:-1], st)                             # shapes
    with pytest.raises(ValueError):
        f(A, dt, st[:-1])
    with pytest.raises(ValueError):
        f(A, st, dt)                                  # the endpoints swapped on a 60 x 50 pattern
    with pytest.raises(ValueError):
        f(A, dt, st[:, :1])                           # heads
    with pytest.raises(ValueError):
        f(A, dt, st[:, :, :4])                        # d
    with pytest.raises(ValueError):
        f(A, dt, st[:, 0])                            # ranks
    with pytest.raises(ValueError):
        f(A, dt[:, 0, 0], st[:, 0, 0])                # 1-D
    with pytest.raises(ValueError):
        f(A, dt[:, :, :0], st[:, :, :0])              # no columns
    assert same(f(A, dt, st).cpu().numpy(), dot_ref(rp, ci, xd.reshape(M, H * d), xs.reshape(K, H * d), H, d))
    assert torch_op.cache_info()["entries"] == 1
    torch_op.clear_cache()
