"""The bf16 edge tensors in the torch front end: edge_op_bf16.edge_op_bf16() and spmm_edge() with a bf16 E.
  Every comparison is on bits, against the fp32 op on the widened tensors: a bf16 result is that op's fp32 result rounded by torch
(.to(bfloat16): round to nearest even), an fp32 result is that op's result.  No NaN occurs in these operands, so plain bit equality
is asked.
  Calls are counted by wrapping the eight Engine methods (the four fp32 entries, the four bf16 ones).
  Peak memory: derived, not measured.  With S = nnz * N elements, forward + backward of edge_op with E holds at the least, on the fp32
route, Z (4S bytes) + the upstream gradient (4S) + E's gradient in E's dtype (2S) and, on the bf16 route, Z (2S) + at most a copy of the
upstream gradient that autograd's accumulation may take (2S) -- everything of node size is the same on both.  spmm_edge: the fp32 E (4S)
and dE (4S) against dE in bf16 (2S).  The bf16 E and upstream gradient themselves exist before either route starts and are not counted.
Either difference is 6S; the test asks for one fp32 tensor, 4S."""
import numpy as np
import pytest

from test_edge_op_gpu import OPS, grads_of
from test_edge_op_torch_gpu import K, M, case
from test_fused_attention_gpu import rand
from test_torch_attention_gpu import make_A
from util import random_csr

pytestmark = pytest.mark.gpu

ENTRIES = ("edge_op_device_rm", "edge_op_backward_device_rm", "spmm_edge_device_rm", "spmm_edge_backward_device_rm")


def bits(t):
    """a tensor's bit patterns on the host: int16 for bf16, int32 for fp32"""
    import torch
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy()


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture
def calls(monkeypatch):
    """name -> how often the Engine method ran"""
    from sextans_amd import api
    count = {}
    for base in ENTRIES:
        for name in (base, base + "_bf16"):
            def wrapped(self, *a, _f=getattr(api.Engine, name), _n=name, **kw):
                count[_n] = count.get(_n, 0) + 1
                return _f(self, *a, **kw)
            monkeypatch.setattr(api.Engine, name, wrapped)
    return count


def engine():
    from sextans_amd import torch_op
    return list(torch_op._cache.values())[-1].eng


def bf16_of(x):
    """numpy fp32 -> a bf16 CUDA tensor (rounded by torch)"""
    import torch
    return torch.from_numpy(x).cuda().to(torch.bfloat16)


# --- edge_op_bf16() -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [5, 16])
@pytest.mark.parametrize("with_e", [False, True])
@pytest.mark.parametrize("op", list(OPS))
def test_edge_op_bits_calls_and_gradients(sx, calls, op, with_e, N):
    """N = 16: everything is read and written where it lies; N = 5: the padded copies, the same contract"""
    import torch
    from sextans_amd import torch_op
    from sextans_amd.edge_op import edge_op
    from sextans_amd.edge_op_bf16 import edge_op_bf16
    rp, ci, v, xd, xs, E, Gz = case(N)
    nnz = len(ci)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    G16, E16 = bf16_of(Gz), bf16_of(E)
    node = lambda x, name: torch.from_numpy(x).cuda().requires_grad_() if name in grads_of(op) else None   # noqa: E731
    # the fp32 op on the widened tensors
    rd, rs_, rE = node(xd, "dxdst"), node(xs, "dxsrc"), (E16.float().requires_grad_() if with_e else None)
    ref = edge_op(A, rd, rs_, rE, op=op)
    ref.backward(G16.float())
    assert ref.dtype == torch.float32 and calls == {"edge_op_device_rm": 1, "edge_op_backward_device_rm": 1}, calls
    calls.clear()
    # the bf16 route
    d, s, Et = node(xd, "dxdst"), node(xs, "dxsrc"), (E16.clone().requires_grad_() if with_e else None)
    seen = []
    if with_e:
        Et.register_hook(lambda g: seen.append((g.data_ptr(), g.dtype)))
    out = edge_op_bf16(A, d, s, Et, op=op)
    assert out.dtype == torch.bfloat16 and out.shape == (nnz, N) and out.requires_grad
    assert engine().last_kernel() == "edge_op_bf16"
    assert same_bits(out, ref.detach().to(torch.bfloat16)), op
    out.backward(G16)
    assert calls == {"edge_op_device_rm_bf16": 1, "edge_op_backward_device_rm_bf16": 1}, calls
    assert engine().last_kernel() == "edge_op_backward_bf16"
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0 and info["entries"] == 1, info
    for g, r in ((d, rd), (s, rs_)):
        if g is not None:
            assert g.grad.dtype == torch.float32 and same_bits(g.grad, r.grad), op
    if with_e:
        assert seen == [(G16.data_ptr(), torch.bfloat16)]          # dE is the upstream gradient itself
        assert same_bits(Et.grad, G16) and same_bits(Et.grad, rE.grad.to(torch.bfloat16))
    # without autograd: the same bits, one more forward call
    with torch.no_grad():
        assert same_bits(edge_op_bf16(A, d, s, Et, op=op), out)
    assert calls["edge_op_device_rm_bf16"] == 2
    torch_op.clear_cache()


def test_edge_op_trailing_shapes_dtypes_and_misuse(sx, calls):
    import torch
    from sextans_amd import torch_op
    from sextans_amd.edge_op import edge_op
    from sextans_amd.edge_op_bf16 import edge_op_bf16
    N, op = 16, "sub"
    rp, ci, v, xd, xs, E, Gz = case(N)
    nnz = len(ci)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    G16, E16 = bf16_of(Gz), bf16_of(E)
    dt, st = torch.from_numpy(xd).cuda(), torch.from_numpy(xs).cuda()
    flat = edge_op_bf16(A, dt, st, E16, op=op)
    # any trailing shape
    d3, s3, E3 = dt.reshape(-1, 2, 8).requires_grad_(), st.reshape(-1, 2, 8).requires_grad_(), E16.reshape(-1, 2, 8).requires_grad_()
    out = edge_op_bf16(A, d3, s3, E3, op=op)
    assert out.shape == (nnz, 2, 8) and out.dtype == torch.bfloat16 and same_bits(out.reshape(nnz, N), flat)
    out.backward(G16.reshape(nnz, 2, 8))
    d2, s2 = dt.clone().requires_grad_(), st.clone().requires_grad_()
    edge_op(A, d2, s2, E16.float(), op=op).backward(G16.float())
    assert same_bits(d3.grad.reshape(-1, N), d2.grad) and same_bits(s3.grad.reshape(-1, N), s2.grad)
    assert E3.grad.shape == E3.shape and same_bits(E3.grad.reshape(nnz, N), G16)
    # node operands in another dtype are widened by torch; their gradients come back in that dtype
    dh, sh = dt.to(torch.bfloat16).requires_grad_(), st.to(torch.bfloat16).requires_grad_()
    out = edge_op_bf16(A, dh, sh, E16, op=op)
    want = edge_op(A, dh.detach().float(), sh.detach().float(), E16.float(), op=op)
    assert same_bits(out, want.to(torch.bfloat16))
    out.backward(G16)
    assert dh.grad.dtype == torch.bfloat16 and sh.grad.dtype == torch.bfloat16
    # an upstream gradient with zero strides (.sum()): a bf16 copy, the fp32 op's bits on ones
    d4, d5 = dt.clone().requires_grad_(), dt.clone().requires_grad_()
    edge_op_bf16(A, d4, st, op=op).sum().backward()
    edge_op(A, d5, st, op=op).sum().backward()
    assert same_bits(d4.grad, d5.grad)
    # misuse: one dtype for all edge tensors of a call, and a bf16 E is read where it lies
    with pytest.raises(ValueError):
        edge_op_bf16(A, dt, st, E16.float(), op=op)
    with pytest.raises(ValueError):
        edge_op_bf16(A, dt, st, E16.to(torch.float16), op=op)
    wide = torch.zeros((nnz, N + 1), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError):
        edge_op_bf16(A, dt, st, wide[:, :N], op=op)     # a row stride the kernel cannot read
    # edge_op() itself: today's route and dtype, whatever E's dtype
    assert edge_op(A, dt, st, E16, op=op).dtype == torch.float32 and engine().last_kernel() == "edge_op"
    assert not any(k.startswith("spmm_edge") for k in calls)
    torch_op.clear_cache()


# --- spmm_edge with a bf16 E -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["mul", "add", "add_relu", "copy"])
def test_spmm_edge_bf16_E_has_the_bits_of_the_route_through_fp32(sx, calls, op):
    import torch
    from sextans_amd import torch_op
    N = 16
    rp, ci, v, _, xs, E, _ = case(N)
    G = rand(np.random.RandomState(7), M, N)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    E16, Gt = bf16_of(E), torch.from_numpy(G).cuda()
    newB = lambda: torch.from_numpy(xs).cuda().requires_grad_() if op != "copy" else None   # noqa: E731
    # the route of the parent commit: the fp32 op on E.float(), the gradient cast to E's dtype
    rB, rE = newB(), E16.float().requires_grad_()
    rC = torch_op.spmm_edge(A, rB, rE, op=op)
    assert engine().last_kernel() == "spmm_edge"
    rC.backward(Gt)
    assert engine().last_kernel() == "spmm_edge_backward"
    assert calls == {"spmm_edge_device_rm": 1, "spmm_edge_backward_device_rm": 1}, calls
    calls.clear()
    B, Et = newB(), E16.clone().requires_grad_()
    C = torch_op.spmm_edge(A, B, Et, op=op)
    assert engine().last_kernel() == "spmm_edge_bf16" and C.dtype == torch.float32
    C.backward(Gt)
    assert engine().last_kernel() == "spmm_edge_backward_bf16"
    assert calls == {"spmm_edge_device_rm_bf16": 1, "spmm_edge_backward_device_rm_bf16": 1}, calls
    assert same_bits(C, rC), op
    assert Et.grad.dtype == torch.bfloat16 and same_bits(Et.grad, rE.grad.to(torch.bfloat16)), op
    if op != "copy":
        assert same_bits(B.grad, rB.grad), op
    # reduce="mean" composes as before; a trailing shape; without autograd
    with torch.no_grad():
        mean = torch_op.spmm_edge(A, B, Et, op=op, reduce="mean")
        assert same_bits(mean, torch_op.spmm_edge(A, rB, rE, op=op, reduce="mean"))
        B3 = B.reshape(K, 2, 8) if B is not None else None
        assert same_bits(torch_op.spmm_edge(A, B3, Et.reshape(-1, 2, 8), op=op).reshape(M, N), rC)
    assert engine().last_kernel() == "spmm_edge_bf16"
    # a bf16 E the kernel cannot read where it lies (N = 5) takes the fp32 copy, as before
    E5 = E16[:, :5].clone().requires_grad_()
    B5 = B.detach()[:, :5].clone() if B is not None else None
    C5 = torch_op.spmm_edge(A, B5, E5, op=op)
    assert engine().last_kernel() == "spmm_edge"
    C5.backward(Gt[:, :5])
    assert engine().last_kernel() == "spmm_edge_backward" and E5.grad.dtype == torch.bfloat16
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0 and info["entries"] == 1, info
    torch_op.clear_cache()


# --- peak memory -----------------------------------------------------------------------------------------------------------------------------
def peak_of(f):
    """the peak of torch's allocated bytes over f() above what is allocated before it"""
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    f()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def test_peak_memory_of_forward_and_backward(sx):
    import torch
    from sextans_amd import torch_op
    from sextans_amd.edge_op import edge_op
    from sextans_amd.edge_op_bf16 import edge_op_bf16
    Mn, N = 2000, 64
    rs = np.random.RandomState(11)
    rp, ci, v = random_csr(rs, Mn, Mn, 20, empty_frac=0.0)
    nnz = len(ci)
    S = nnz * N
    assert 2_000_000 <= S <= 4_000_000
    torch_op.clear_cache()
    A = make_A(rp, ci, v, Mn, Mn)
    x = torch.from_numpy(rand(rs, Mn, N)).cuda()
    E16, G16 = bf16_of(rand(rs, nnz, N)), bf16_of(rand(rs, nnz, N))
    Gn = torch.from_numpy(rand(rs, Mn, N)).cuda()

    def op_fp32():      # what the parent commit does with a bf16 edge_attr: fp32 Z, fp32 upstream gradient
        d, s, e = x.clone().requires_grad_(), x.clone().requires_grad_(), E16.detach().requires_grad_()
        edge_op(A, d, s, e, op="add").backward(G16.float())

    def op_bf16():
        d, s, e = x.clone().requires_grad_(), x.clone().requires_grad_(), E16.detach().requires_grad_()
        edge_op_bf16(A, d, s, e, op="add").backward(G16)

    def edge_fp32():    # the fp32 op on E.float()
        b, e = x.clone().requires_grad_(), E16.float().requires_grad_()
        torch_op.spmm_edge(A, b, e, op="mul").backward(Gn)

    def edge_bf16():
        b, e = x.clone().requires_grad_(), E16.detach().requires_grad_()
        torch_op.spmm_edge(A, b, e, op="mul").backward(Gn)

    for f32, f16, what in ((op_fp32, op_bf16, "edge_op"), (edge_fp32, edge_bf16, "spmm_edge")):
        f32(), f16()                      # (the engine, A^T and torch's own one-time allocations)
        p32, p16 = peak_of(f32), peak_of(f16)
        print(what, "peak bytes fp32 route", p32, "bf16 route", p16, "difference / (4 S)", (p32 - p16) / (4.0 * S))
        assert p32 - p16 >= 4 * S, what
    torch_op.clear_cache()
