"""sextans_amd.edge_op.edge_op on the GPU: forward and the gradients of x_dst, x_src and E against the torch composition
x_dst[rows] (op) x_src[cols] + E in float64 (gathers by entry_rows / col_indices, autograd through index_add_) on a 60 x 50 random pattern
with empty rows, N = 5 (no multiple of 8: the padded copies) and N = 16; trailing shapes and non-contiguous operands; x_dst is x_src on a
square pattern; only the gradients asked for, the skipped pass shown by last_kernel on a pattern whose long rows are on one side; misuse.
  Tolerances, derived: the forward is r2 = fl(fl(z1) + E) with z1 = x_dst (op) x_src exact in float64, so |r2 - (z1 + E)| <=
2^-24 (2 |z1| + |E|) to first order (a factor 1.001 covers the second-order term); it also has the bits of the float32 composition.
The gradients: (n + 2) 2^-24 sum |t_e|, the bound of test_edge_op_gpu.py."""
import numpy as np
import pytest

from test_edge_op_gpu import OPS, backward_ref, grads_of, within_bound
from test_fused_attention_gpu import rand, same
from test_pattern_dealing_gpu import pat
from test_torch_attention_gpu import make_A
from util import random_csr

pytestmark = pytest.mark.gpu

M, K = 60, 50
U = 2.0 ** -24
_cases = {}


def case(N):
    """the pattern (empty rows among its 60) with x_dst, x_src, E and the upstream gradient in +-1, once per N"""
    if N not in _cases:
        rs = np.random.RandomState(61)
        rp, ci, v = random_csr(rs, M, K, 6, empty_frac=0.15)
        assert 3 <= np.count_nonzero(np.diff(rp) == 0) < M // 2
        nnz = len(ci)
        _cases[N] = (rp, ci, v, rand(rs, M, N), rand(rs, K, N), rand(rs, nnz, N), rand(rs, nnz, N))
    return _cases[N]


def compose(op, A, xd, xs, E):
    """the torch composition in the operands' dtype: two gathers, one elementwise pass, autograd through index_add_"""
    from sextans_amd import torch_op
    rows, cols = torch_op.entry_rows(A), A.col_indices().long()
    d = xd[rows] if xd is not None else None
    s = xs[cols] if xs is not None else None
    z = d + s if op == "add" else d - s if op == "sub" else d * s if op == "mul" else d if op == "dst" else s
    return z + E if E is not None else z


def operands(op, xd, xs, E, with_e, grad=True, dtype=None):
    import torch
    t = lambda x: (torch.from_numpy(x).cuda().to(dtype) if dtype else torch.from_numpy(x).cuda()).requires_grad_(grad)   # noqa: E731
    return (t(xd) if op != "src" else None), (t(xs) if op != "dst" else None), (t(E) if with_e else None)


@pytest.mark.parametrize("N", [5, 16])
@pytest.mark.parametrize("with_e", [False, True])
@pytest.mark.parametrize("op", list(OPS))
def test_forward_and_gradients(sx, op, with_e, N):
    import torch
    from sextans_amd import torch_op
    from sextans_amd.edge_op import edge_op
    rp, ci, v, xd, xs, E, Gz = case(N)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    Gt = torch.from_numpy(Gz).cuda()
    ref = operands(op, xd, xs, E, with_e, dtype=torch.float64)
    want = compose(op, A, *ref)
    want.backward(Gt.double())
    got = operands(op, xd, xs, E, with_e)
    out = edge_op(A, *got, op=op)
    assert out.requires_grad and out.shape == (len(ci), N) and out.dtype == torch.float32
    out.backward(Gt)
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0 and info["entries"] == 1, info
    # forward: the derived bound against float64, the bits of the float32 composition
    z1 = (want.detach() - ref[2].detach() if with_e else want.detach()).abs().cpu().numpy()
    bound = 1.001 * U * (2 * z1 + (np.abs(E) if with_e else 0))
    err = np.abs(out.detach().cpu().numpy().astype(np.float64) - want.detach().cpu().numpy())
    print(op, with_e, N, "forward max err / bound", float((err[bound > 0] / bound[bound > 0]).max()))
    assert np.all(err <= bound)
    with torch.no_grad():
        plain = compose(op, A, *(None if x is None else x.detach() for x in got))
        assert same(out.detach().cpu().numpy(), plain.cpu().numpy())
        assert same(edge_op(A, *got, op=op).cpu().numpy(), plain.cpu().numpy())   # without autograd: the same bits
    # gradients
    _, mags, counts = backward_ref(op, rp, ci, xd, xs, Gz, M, K)
    for name, g, r in (("dxdst", got[0], ref[0]), ("dxsrc", got[1], ref[1])):
        assert (g is None) == (name not in grads_of(op))
        if g is not None:
            assert g.grad.shape == g.shape and g.grad.dtype == torch.float32
            assert within_bound(g.grad.cpu().numpy(), r.grad.cpu().numpy(), mags[name], counts[name], "%s %s N=%d" % (op, name, N)), name
            assert np.all(g.grad.cpu().numpy()[counts[name] == 0] == 0)
    if with_e:
        assert same(got[2].grad.cpu().numpy(), Gz) and np.array_equal(ref[2].grad.cpu().numpy(), Gz.astype(np.float64))
    # .sum().backward(): an upstream gradient with zero strides
    again = operands(op, xd, xs, E, with_e)
    edge_op(A, *again, op=op).sum().backward()
    _, mags1, _ = backward_ref(op, rp, ci, xd, xs, np.ones_like(Gz), M, K)
    ones = operands(op, xd, xs, E, with_e, dtype=torch.float64)
    compose(op, A, *ones).sum().backward()
    for name, g, r in (("dxdst", again[0], ones[0]), ("dxsrc", again[1], ones[1])):
        if g is not None:
            assert within_bound(g.grad.cpu().numpy(), r.grad.cpu().numpy(), mags1[name], counts[name], "sum " + name), name
    assert torch_op.cache_info() == info
    torch_op.clear_cache()


def test_trailing_shapes_and_non_contiguous_operands(sx):
    """operands with a (., 2, 8) trailing shape; column slices of wider tensors, a transposed x_src, an E with a row stride the kernel
    cannot read"""
    import torch
    from sextans_amd import torch_op
    from sextans_amd.edge_op import edge_op
    N, op = 16, "sub"
    rp, ci, v, xd, xs, E, Gz = case(N)
    nnz = len(ci)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    Gt = torch.from_numpy(Gz).cuda()
    dt, st, Et = operands(op, xd, xs, E, True)
    flat = edge_op(A, dt, st, Et, op=op)
    flat.backward(Gt)
    d3, s3, E3 = (x.detach().reshape(-1, 2, 8).requires_grad_() for x in (dt, st, Et))
    out = edge_op(A, d3, s3, E3, op=op)
    assert out.shape == (nnz, 2, 8)
    out.backward(Gt.reshape(nnz, 2, 8))
    assert same(out.detach().reshape(nnz, N).cpu().numpy(), flat.detach().cpu().numpy())
    for x3, x in ((d3, dt), (s3, st), (E3, Et)):
        assert x3.grad.shape == x3.shape and same(x3.grad.reshape(-1, N).cpu().numpy(), x.grad.cpu().numpy())
    dw = torch.zeros((M, 2 * N), device="cuda")
    dw[:, ::2] = dt.detach()
    sw = st.detach().t().contiguous().t()
    Ew = torch.zeros((nnz, N + 1), device="cuda")
    Ew[:, :N] = Et.detach()
    dn, sn, En = dw[:, ::2].requires_grad_(), sw.requires_grad_(), Ew[:, :N].requires_grad_()
    assert not dn.is_contiguous() and not sn.is_contiguous() and not En.is_contiguous()
    out = edge_op(A, dn, sn, En, op=op)
    out.backward(Gt[:, :].t().contiguous().t())   # a non-contiguous upstream gradient too
    assert same(out.detach().cpu().numpy(), flat.detach().cpu().numpy())
    for xn, x in ((dn, dt), (sn, st), (En, Et)):
        assert same(xn.grad.cpu().numpy(), x.grad.cpu().numpy())
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0 and info["entries"] == 1, info
    torch_op.clear_cache()


@pytest.mark.parametrize("op", ["add", "sub", "mul"])
def test_x_dst_is_x_src(sx, op):
    """one tensor for both endpoints of a square pattern: its gradient is the sum of both passes"""
    import torch
    from sextans_amd import torch_op
    from sextans_amd.edge_op import edge_op
    N, n = 16, 50
    rs = np.random.RandomState(62)
    rp, ci, v = random_csr(rs, n, n, 6, empty_frac=0.15)
    x, Gz = rand(rs, n, N), rand(rs, len(ci), N)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, n, n)
    Gt = torch.from_numpy(Gz).cuda()
    xt = torch.from_numpy(x).cuda().requires_grad_()
    out = edge_op(A, xt, xt, op=op)
    out.backward(Gt)
    a, b = (torch.from_numpy(x).cuda().requires_grad_() for _ in range(2))
    two = edge_op(A, a, b, op=op)
    two.backward(Gt)
    assert same(out.detach().cpu().numpy(), two.detach().cpu().numpy())
    assert same(xt.grad.cpu().numpy(), (a.grad + b.grad).cpu().numpy())
    x64 = torch.from_numpy(x).cuda().double().requires_grad_()
    compose(op, A, x64, x64, None).backward(Gt.double())
    _, mags, counts = backward_ref(op, rp, ci, x, x, Gz, n, n)
    bound = ((counts["dxdst"] + 2)[:, None] * mags["dxdst"] + (counts["dxsrc"] + 2)[:, None] * mags["dxsrc"]) * U + \
        U * np.abs(x64.grad.cpu().numpy())   # both passes' bounds and the rounding of their sum
    assert np.all(np.abs(xt.grad.cpu().numpy().astype(np.float64) - x64.grad.cpu().numpy()) <= 1.001 * bound)
    torch_op.clear_cache()


def test_only_the_gradients_asked_for(sx):
    """each requires_grad subset returns only what is asked, with the bits of the full call; on pattern P (long rows in P, none in P^T)
    last_kernel names the pass that ran: dx_dst alone walks P (+long_rows) and builds no A^T, dx_src alone walks P^T"""
    import itertools
    import torch
    from sextans_amd import torch_op
    from sextans_amd.edge_op import edge_op
    N, op = 8, "mul"
    p = pat("P")
    rs = np.random.RandomState(63)
    xd, xs, E, Gz = rand(rs, p.M, N), rand(rs, p.K, N), rand(rs, p.nnz, N), rand(rs, p.nnz, N)
    torch_op.clear_cache()
    A = make_A(p.rp, p.ci, np.ones(p.nnz, np.float32), p.M, p.K)
    eng = lambda: list(torch_op._cache.values())[-1].eng   # noqa: E731
    Gt = torch.from_numpy(Gz).cuda()
    t = lambda x, g: torch.from_numpy(x).cuda().requires_grad_(g)   # noqa: E731
    # E alone: no backward call at all; x_dst alone: no A^T
    ops = [t(xd, False), t(xs, False), t(E, True)]
    edge_op(A, *ops, op=op).backward(Gt)
    assert eng().last_kernel() == "edge_op+long_rows" and same(ops[2].grad.cpu().numpy(), Gz)   # (the upstream gradient itself)
    ops = [t(xd, True), t(xs, False), t(E, False)]
    edge_op(A, *ops, op=op).backward(Gt)
    assert eng().last_kernel() == "edge_op_backward+long_rows" and eng().get_stat("transpose_build_s") == 0
    ops = [t(xd, False), t(xs, True), t(E, False)]
    edge_op(A, *ops, op=op).backward(Gt)
    assert eng().last_kernel() == "edge_op_backward" and eng().get_stat("transpose_build_s") > 0
    full = [t(xd, True), t(xs, True), t(E, True)]
    edge_op(A, *full, op=op).backward(Gt)
    assert eng().last_kernel() == "edge_op_backward+long_rows"
    for k in range(4):
        for subset in itertools.combinations(range(3), k):
            ops = [x.detach().clone().requires_grad_(i in subset) for i, x in enumerate(full)]
            out = edge_op(A, *ops, op=op)
            assert out.requires_grad == bool(subset)
            if subset:
                out.backward(Gt)
            for i, x in enumerate(ops):
                if i in subset:
                    assert same(x.grad.cpu().numpy(), full[i].grad.cpu().numpy()), (subset, i)
                else:
                    assert x.grad is None, (subset, i)
    # A gets no gradient even when it asks
    Ag = make_A(p.rp, p.ci, np.ones(p.nnz, np.float32), p.M, p.K, grad=True)
    edge_op(Ag, *[x.detach().requires_grad_() for x in full], op=op).backward(Gt)
    assert Ag.grad is None
    # not twice differentiable
    ops = [x.detach().requires_grad_() for x in full]
    g, = torch.autograd.grad(edge_op(A, *ops, op=op), ops[0], Gt, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    torch_op.clear_cache()


def test_misuse(sx):
    from sextans_amd import torch_op
    from sextans_amd.edge_op import edge_op as f
    N = 16
    rp, ci, v, xd, xs, E, Gz = case(N)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    dt, st, Et = operands("add", xd, xs, E, True, grad=False)
    with pytest.raises(ValueError):
        f(A, dt, st, op="div")                    # an unknown op
    with pytest.raises(ValueError):
        f(A, dt, st, op=1)
    for op in ("add", "sub", "mul", "dst"):
        with pytest.raises(ValueError):
            f(A, None, st, op=op)                 # a missing operand the op reads
    for op in ("add", "sub", "mul", "src"):
        with pytest.raises(ValueError):
            f(A, dt, None, op=op)
    with pytest.raises(ValueError):
        f(A, None, None, Et, op="add")
    with pytest.raises(TypeError):
        f(A, dt.cpu(), st)                        # CPU operands
    with pytest.raises(TypeError):
        f(A, dt, st.cpu())
    with pytest.raises(TypeError):
        f(A, dt, st, Et.cpu())
    with pytest.raises(TypeError):
        f(A.to_dense(), dt, st)                   # a dense A
    with pytest.raises(TypeError):
        f(A, dt, st.to_sparse())                  # a sparse operand
    with pytest.raises(ValueError):
        f(A, dt[:-1], st)                         # shapes
    with pytest.raises(ValueError):
        f(A, dt, st[:-1])
    with pytest.raises(ValueError):
        f(A, dt, st, Et[:-1])
    with pytest.raises(ValueError):
        f(A, st, dt)                              # the endpoints swapped on a 60 x 50 pattern
    with pytest.raises(ValueError):
        f(A, dt, st[:, :8])
    with pytest.raises(ValueError):
        f(A, dt, st, Et.reshape(-1, 2, 8))
    with pytest.raises(ValueError):
        f(A, dt[:, 0], st[:, 0])                  # 1-D
    with pytest.raises(ValueError):
        f(A, dt[:, :0], st[:, :0])                # no columns
    # the operand an op does not read is ignored, whatever it is
    assert same(f(A, dt, None, op="dst").cpu().numpy(), f(A, dt, st[:3], op="dst").cpu().numpy())
    assert same(f(A, None, st, op="src").cpu().numpy(), f(A, "nothing", st, op="src").cpu().numpy())
    assert torch_op.cache_info()["entries"] == 1
    torch_op.clear_cache()
