"""The bf16 edge tensors of the gated aggregation in the torch front end, on the 400 x 300 matrix of the reduce tests:
  gated.spmm_gated() with a qualifying bf16 E and return_edge=False takes the bf16 entry points by itself and returns the bits of the
route through the fp32 copies -- forced here with an E of the same values whose base lies 8 bytes behind an aligned address, or that
is not row-major --; with return_edge=True it keeps the copies and the fp32 z;
  gated_bf16.spmm_gated_bf16() returns z in bf16 and reads E and the upstream gradient of z where they lie: C, z and the gradients
are those of spmm_gated(..., E.float(), return_edge=True) with z.to(bfloat16), the upstream gradient of z widened and E's gradient
rounded once.
Every comparison is on bits.  Which kernels ran is read from last_kernel."""
import numpy as np
import pytest

from test_edge_bf16_torch_gpu import bf16_of, engine, same_bits
from test_fused_attention_gpu import rand
from test_spmm_reduce_gpu import base_matrix
from test_torch_attention_gpu import make_A

pytestmark = pytest.mark.gpu

_cases = {}


def case(N):
    """the matrix and, as numpy fp32, x_dst, x_src, V, E, G and Gz; once per N, never changed"""
    if N not in _cases:
        rs, rp, ci, v, M, K = base_matrix(5)
        nnz = len(ci)
        _cases[N] = (rp, ci, v, M, K, rand(rs, M, N), rand(rs, K, N), rand(rs, K, N), rand(rs, nnz, N), rand(rs, M, N), rand(rs, nnz, N))
    return _cases[N]


def leaves(*xs):
    """numpy or tensors -> fresh CUDA leaves that require grad (None stays None)"""
    import torch
    out = []
    for x in xs:
        t = None if x is None else (torch.from_numpy(x).cuda() if isinstance(x, np.ndarray) else x.detach().clone())
        out.append(t.requires_grad_() if t is not None else None)
    return out


def offset_by_8_bytes(E16):
    """the same values in a row-major tensor whose first element lies 8 bytes behind an aligned address: the kernel cannot read it"""
    import torch
    buf = torch.empty((E16.numel() + 4,), dtype=torch.bfloat16, device="cuda")
    out = buf[4:].view(E16.shape)
    out.copy_(E16)
    assert out.data_ptr() % 16 == 8
    return out.requires_grad_()


def column_major(E16):
    return E16.detach().t().contiguous().t().requires_grad_()


@pytest.mark.parametrize("other", [offset_by_8_bytes, column_major])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("N", [16, 24])
def test_spmm_gated_takes_the_bf16_kernels_and_returns_the_bits_of_the_copy_route(sx, N, normalize, other):
    import torch
    from sextans_amd import torch_op
    from sextans_amd.gated import spmm_gated
    rp, ci, v, M, K, xd, xs, V, E, G, _ = case(N)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    E16, Gt = bf16_of(E), torch.from_numpy(G).cuda()
    # the copy route: an E of the same values that the kernel cannot read where it lies
    r = leaves(xd, xs, V) + [other(E16)]
    assert same_bits(r[3], E16)
    rC = spmm_gated(A, *r, normalize=normalize)
    assert engine().last_kernel() == "spmm_gated"
    rC.backward(Gt)
    assert engine().last_kernel() == "spmm_gated_backward" and r[3].grad.dtype == torch.bfloat16
    # the native route
    t = leaves(xd, xs, V, E16)
    C = spmm_gated(A, *t, normalize=normalize)
    assert engine().last_kernel() == "spmm_gated_bf16"
    assert C.dtype == torch.float32 and same_bits(C, rC)
    C.backward(Gt)
    assert engine().last_kernel() == "spmm_gated_backward_bf16"
    for name, a, b in zip(("x_dst", "x_src", "V", "E"), t, r):
        assert a.grad.dtype == a.dtype and same_bits(a.grad, b.grad), name
    assert t[3].grad.dtype == torch.bfloat16 and bool(t[3].grad.float().abs().max() > 0)
    with torch.no_grad():   # without autograd: the same route, the same bits
        assert same_bits(spmm_gated(A, *t, normalize=normalize), C) and engine().last_kernel() == "spmm_gated_bf16"
    # return_edge=True keeps the fp32 z and the copies: the old bits
    t2 = leaves(xd, xs, V, E16)
    C2, z2 = spmm_gated(A, *t2, normalize=normalize, return_edge=True)
    assert engine().last_kernel() == "spmm_gated" and z2.dtype == torch.float32 and same_bits(C2, rC)
    w = leaves(xd, xs, V, E16.float())
    wC, wz = spmm_gated(A, *w, normalize=normalize, return_edge=True)
    assert same_bits(z2, wz)
    Gz = torch.from_numpy(case(N)[10]).cuda()
    torch.autograd.backward([C2, z2], [Gt, Gz])
    assert engine().last_kernel() == "spmm_gated_backward"
    torch.autograd.backward([wC, wz], [Gt, Gz])
    for name, a, b in zip(("x_dst", "x_src", "V"), t2, w):
        assert same_bits(a.grad, b.grad), name
    assert same_bits(t2[3].grad, w[3].grad.to(torch.bfloat16))
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0, info
    torch_op.clear_cache()


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("N", [16, 20, 24])
def test_spmm_gated_bf16_is_spmm_gated_with_z_and_the_edge_gradients_rounded_once(sx, N, normalize):
    """N = 16, 24: everything is read and written where it lies; N = 20: the zero-padded bf16 copies, the same contract"""
    import torch
    from sextans_amd import torch_op
    from sextans_amd.gated import spmm_gated
    from sextans_amd.gated_bf16 import spmm_gated_bf16
    rp, ci, v, M, K, xd, xs, V, E, G, Gz = case(N)
    nnz = len(ci)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    E16, Gz16, Gt = bf16_of(E), bf16_of(Gz), torch.from_numpy(G).cuda()
    w = leaves(xd, xs, V, E16.float())
    wC, wz = spmm_gated(A, *w, normalize=normalize, return_edge=True)
    torch.autograd.backward([wC, wz], [Gt, Gz16.float()])
    t = leaves(xd, xs, V, E16)
    C, z = spmm_gated_bf16(A, *t, normalize=normalize, return_edge=True)
    assert engine().last_kernel() == "spmm_gated_bf16"
    assert C.dtype == torch.float32 and z.dtype == torch.bfloat16 and z.shape == (nnz, N) and C.requires_grad and z.requires_grad
    assert same_bits(C, wC) and same_bits(z, wz.to(torch.bfloat16))
    assert not same_bits(z.float(), wz)                                   # (the rounding is not vacuous)
    torch.autograd.backward([C, z], [Gt, Gz16])
    assert engine().last_kernel() == "spmm_gated_backward_bf16"
    for name, a, b in zip(("x_dst", "x_src", "V"), t, w):
        assert a.grad.dtype == torch.float32 and same_bits(a.grad, b.grad), name
    assert t[3].grad.dtype == torch.bfloat16 and same_bits(t[3].grad, w[3].grad.to(torch.bfloat16))
    # only z used downstream; return_edge=False; no autograd
    t3 = leaves(xd, xs, V, E16)
    _, z3 = spmm_gated_bf16(A, *t3, normalize=normalize, return_edge=True)
    z3.backward(Gz16)
    assert same_bits(z3, z) and same_bits(t3[3].grad, Gz16) and not t3[2].grad.any()
    assert same_bits(spmm_gated_bf16(A, *t, normalize=normalize), C)
    with torch.no_grad():
        C4, z4 = spmm_gated_bf16(A, *t, normalize=normalize, return_edge=True)
    assert same_bits(C4, C) and same_bits(z4, z) and engine().last_kernel() == "spmm_gated_bf16"
    # E=None: a bf16 z all the same, differentiable through both outputs
    t5, w5 = leaves(xd, xs, V), leaves(xd, xs, V)
    C5, z5 = spmm_gated_bf16(A, *t5, normalize=normalize, return_edge=True)
    assert engine().last_kernel() == "spmm_gated_bf16"
    wC5, wz5 = spmm_gated(A, *w5, normalize=normalize, return_edge=True)
    assert z5.dtype == torch.bfloat16 and same_bits(C5, wC5) and same_bits(z5, wz5.to(torch.bfloat16))
    torch.autograd.backward([C5, z5], [Gt, Gz16])
    torch.autograd.backward([wC5, wz5], [Gt, Gz16.float()])
    for name, a, b in zip(("x_dst", "x_src", "V"), t5, w5):
        assert same_bits(a.grad, b.grad), name
    # a bf16 E that is not row-major takes a bf16 copy; any other dtype is refused
    t6 = leaves(xd, xs, V) + [column_major(E16)]
    C6, z6 = spmm_gated_bf16(A, *t6, normalize=normalize, return_edge=True)
    assert engine().last_kernel() == "spmm_gated_bf16" and same_bits(C6, C) and same_bits(z6, z)
    with pytest.raises(ValueError):
        spmm_gated_bf16(A, *w, normalize=normalize)
    with pytest.raises(ValueError):
        spmm_gated_bf16(A, t[0], t[1], t[2], E16.to(torch.float16))
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0, info
    torch_op.clear_cache()
