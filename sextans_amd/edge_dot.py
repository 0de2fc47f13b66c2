"""Per-head dot product of both endpoints for torch: DGL's u_dot_v (the last member of its gSDDMM set) as one launch over a sparse_csr
pattern for all heads, dealt by non-zeros -- the (nnz, H) scores that torch_op.score_attention() reads, without a per-head sddmm() loop,
without x[rows] and x[cols] materialised and without index_add_'s float atomics in the backward.
Public: edge_dot().  The other ops of the torch front end live in sextans_amd.torch_op and sextans_amd.edge_op; this one shares their
cached engines (torch_op.cache_info() / clear_cache() cover it), the frame of the tiled families in _op_aggregate.py and the heads
operands of the fused families in _op_attention.py."""
import torch
from torch.autograd.function import once_differentiable

from ._op_aggregate import _any_elements, _tiled_entry
from ._op_attention import _heads_operand, _scalars_operand, _with_heads
from ._op_cache import (_check_dense, _check_sparse, _cut_grad, _f32, _index_tensors, _keep_pattern, _kept_pattern_entry,
                        _ptr_nonempty)

__all__ = ["edge_dot"]


def _edge_dot_forward(A, x_dst, x_src, fast):
    """S (nnz, H) of the engine's per-head dot product; x_dst (M, H, d), x_src (K, H, d), d padded up to a multiple of 8 where it must be
    (zero columns, which add +0 at the end of every chain)."""
    H, d = x_dst.shape[1], x_dst.shape[2]
    M, K, dp, ent, stream, val = _tiled_entry(A, d, fast)
    S = _f32(A.device, val.numel(), H)
    if _any_elements(S):
        X, ldx = _heads_operand(x_dst.detach(), dp)
        Y, ldy = (X, ldx) if x_src is x_dst else _heads_operand(x_src.detach(), dp)
        ent.eng.edge_dot_device(H, dp, _ptr_nonempty(X), ldx, _ptr_nonempty(Y), ldy, _ptr_nonempty(S), H, stream)
    return S


class _EdgeDotFunction(torch.autograd.Function):
    """edge_dot(): ONE forward call (sextans_edge_dot_device), ONE backward call (sextans_edge_dot_backward_device) for the gradients
    that are wanted: score_attention's WEIGHT forward over A's rows for x_dst, its WEIGHT column pass over A^T's rows for x_src.  With
    x_dst is x_src the operand comes in once and the two gradients are added.  A's values never enter: no gradient for A, no value
    refresh.  Not twice differentiable."""

    @staticmethod
    def forward(ctx, A, x_dst, x_src, fast):
        same = x_src is None
        S = _edge_dot_forward(A, x_dst, x_dst if same else x_src, fast)
        ctx.save_for_backward(*_index_tensors(A), A.values(), x_dst, *(() if same else (x_src,)))
        _keep_pattern(ctx, A, fast)
        ctx.same = same
        return S

    @staticmethod
    @once_differentiable
    def backward(ctx, Gs):
        crow, col, val, x_dst = ctx.saved_tensors[:4]
        x_src = x_dst if ctx.same else ctx.saved_tensors[4]
        M, K = ctx.shape
        H, d = x_dst.shape[1], x_dst.shape[2]
        dp = -(-d // 8) * 8
        want_d = ctx.needs_input_grad[1]
        want_s = want_d if ctx.same else ctx.needs_input_grad[2]
        if not (want_d or want_s):
            return None, None, None, None
        dd = _f32(Gs.device, M, H, dp) if want_d else None
        ds = _f32(Gs.device, K, H, dp) if want_s else None
        if _any_elements(dd, ds):
            ent, stream = _kept_pattern_entry(ctx, crow, col, val)
            G, ldg = _scalars_operand(Gs)                       # (a copy when Gs has zero strides, e.g. after .sum())
            X, ldx = _heads_operand(x_dst.detach(), dp) if want_s else (None, H * dp)    # x_dst is read for x_src's gradient alone
            Y, ldy = ((X, ldx) if ctx.same else _heads_operand(x_src.detach(), dp)) if want_d else (None, H * dp)
            ent.eng.edge_dot_backward_device(H, dp, _ptr_nonempty(X), ldx, _ptr_nonempty(Y), ldy, _ptr_nonempty(G), ldg, _ptr_nonempty(dd), H * dp,
                                             _ptr_nonempty(ds), H * dp, stream)
        if ctx.same:
            return None, _cut_grad(dd + ds, d, x_dst), None, None
        return None, _cut_grad(dd, d, x_dst, want_d), _cut_grad(ds, d, x_src, want_s), None


def edge_dot(A, x_dst, x_src, fast=False):
    """One score per stored entry and head from both of its endpoints (DGL's u_dot_v; the producer torch_op.score_attention() lacked):
    for every stored entry e = (r, c) of A, in A's CSR entry order, and every head h
        S[e, h] = < x_dst[r, h, :], x_src[c, h, :] >
    A is an (M, K) sparse_csr matrix of which only the PATTERN is used (its values are not read, the cached engine is not refreshed and A
    gets no gradient); x_dst is (M, H, d) or (M, d), x_src (K, H, d) or (K, d) in the same rank; the result is (nnz, H) or (nnz,), fp32
    (torch_op.entry_rows() gives the row of every entry).  AGNN's cosine score, HGT's K W Q, SuperGAT's dot-product mode and any clamped,
    tempered or MLP-adjusted transformer score are edge_dot, elementwise ops, score_attention; a scale belongs on x_dst or on S.  One
    launch for all heads, dealt by non-zeros (sextans_edge_dot_device): a hub row spreads over many wavefronts, nothing of size
    nnz x H x d exists.  Every product and every sum is rounded to fp32 in the order of d -- per head the bits of
    torch_op.sddmm(A_pattern, x_dst[:, h], x_src[:, h]) on a pattern of ones.  Differentiable in x_dst and x_src: sums over A's rows
    and over A^T's rows in an order fixed by the pattern (sextans_edge_dot_backward_device, the WEIGHT-mode passes of score_attention)
    -- no atomics, the same bits on every run --, and only the passes whose gradients autograd wants are launched; not twice
    differentiable.  x_dst is x_src is fine on a square pattern.  d up to 128; a d that is not a multiple of 8, and operands the
    kernel cannot read where they lie, are copied with zero padding, as edge_op() does; `fast` only selects the cached engine."""
    name = "edge_dot"
    _check_sparse(A, name)
    _check_dense(name, "x_dst and x_src", x_dst, x_src)
    if x_dst.layout != torch.strided or x_src.layout != torch.strided:
        raise TypeError(name + " expects CUDA/HIP dense x_dst and x_src")
    if x_dst.dim() not in (2, 3) or x_src.dim() != x_dst.dim():
        raise ValueError(name + ": x_dst is (M, d) or (M, H, d), x_src (K, d) or (K, H, d), in one rank")
    d3, s3 = _with_heads(x_dst, 3), _with_heads(x_src, 3)
    M, K = A.shape
    H, d = d3.shape[1], d3.shape[2]
    if s3.shape[1:] != d3.shape[1:]:
        raise ValueError(name + ": x_dst and x_src differ in their heads or head dimension")
    if d3.shape[0] != M or s3.shape[0] != K or H == 0 or d == 0:
        raise ValueError("shape mismatch")
    if d > 128:
        raise ValueError(name + ": d up to 128 (split the head dimension and add the parts' scores)")
    same = x_src is x_dst
    if torch.is_grad_enabled() and (d3.requires_grad or s3.requires_grad):
        S = _EdgeDotFunction.apply(A, d3, None if same else s3, bool(fast))
    else:
        S = _edge_dot_forward(A, d3, d3 if same else s3, bool(fast))
    return S if x_dst.dim() == 3 else S[:, 0]
