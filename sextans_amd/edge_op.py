"""Edge-output ops from both endpoints for torch: DGL's u_add_v / u_sub_v / u_mul_v / copy_u / copy_v (gSDDMM, each optionally + e) as one
fused pass over a sparse_csr pattern per direction -- the (nnz, N) tensors that score_attention, vector_attention, spmm_edge* and
spmm_edge_softagg read, without x[rows] and x[cols] materialised and without index_add_'s float atomics in the backward.
Public: edge_op().  The other ops of the torch front end live in sextans_amd.torch_op; this one shares their cached engines
(torch_op.cache_info() / clear_cache() cover it) and the frame of the tiled families in _op_aggregate.py."""
import math

import torch
from torch.autograd.function import once_differentiable

from . import api
from ._op_aggregate import _any_elements, _rowmajor_ld, _tiled_entry
from ._op_cache import (_check_sparse, _cut, _cut_grad, _f32, _index_tensors, _keep_pattern, _kept_pattern_entry, _ptr_nonempty,
                        _qualifies)

__all__ = ["edge_op"]

_OPS = {"add": api.EDGEOP_ADD, "sub": api.EDGEOP_SUB, "mul": api.EDGEOP_MUL, "dst": api.EDGEOP_DST, "src": api.EDGEOP_SRC}


def _edge_op_forward(A, x_dst, x_src, E, op, N, fast, bf16=False):
    """Z (nnz, Np) of the engine's edge op, N padded up to a multiple of 8 (zero columns of the operands, which are cut again); x_dst is
    None for EDGEOP_SRC, x_src for EDGEOP_DST, E when there are no edge features.  bf16: E (a bf16 tensor, or None) and Z in bf16,
    through sextans_edge_op_device_rm_bf16."""
    M, K, Np, ent, stream, val = _tiled_entry(A, N, fast)
    nnz = val.numel()
    e_dtype = torch.bfloat16 if bf16 else torch.float32
    drm, ldd = _rowmajor_ld(x_dst, M, N, Np)
    srm, lds = _rowmajor_ld(x_src, K, N, Np)
    Erm, lde = _rowmajor_ld(E, nnz, N, Np, e_dtype)
    Z = torch.empty((nnz, Np), dtype=e_dtype, device=A.device)
    if _any_elements(Z):
        call = ent.eng.edge_op_device_rm_bf16 if bf16 else ent.eng.edge_op_device_rm
        call(op, Np, _ptr_nonempty(drm), ldd, _ptr_nonempty(srm), lds, _ptr_nonempty(Erm), lde, _ptr_nonempty(Z), Np, stream)
    return Z


class _EdgeOpFunction(torch.autograd.Function):
    """edge_op(): ONE forward call (sextans_edge_op_device_rm), ONE backward call (sextans_edge_op_backward_device_rm) for the endpoint
    gradients that are wanted: a sum over A's rows for x_dst, the same pass over A^T's rows for x_src.  E's gradient is the upstream
    gradient itself.  A's values never enter: no gradient for A, no value refresh.  Not twice differentiable.  bf16: the _bf16 entry
    points -- Z, E and the upstream gradient in bf16, the endpoint gradients fp32 sums as before."""

    @staticmethod
    def forward(ctx, A, x_dst, x_src, E, op, N, fast, bf16=False):
        Z = _edge_op_forward(A, x_dst, x_src, E, op, N, fast, bf16)
        ctx.save_for_backward(*_index_tensors(A), A.values(), x_dst, x_src)
        _keep_pattern(ctx, A, fast)
        ctx.op, ctx.N, ctx.e_dtype, ctx.bf16 = op, N, E.dtype if E is not None else None, bf16
        return _cut(Z, N)

    @staticmethod
    @once_differentiable
    def backward(ctx, Gz):
        crow, col, val, x_dst, x_src = ctx.saved_tensors
        M, K = ctx.shape
        op, N = ctx.op, ctx.N
        nnz, Np = val.numel(), api.round_up_n(N)
        want_d = x_dst is not None and ctx.needs_input_grad[1]
        want_s = x_src is not None and ctx.needs_input_grad[2]
        dE = Gz.to(ctx.e_dtype) if ctx.e_dtype is not None and ctx.needs_input_grad[3] else None   # (E's own dtype: Gz itself, no copy)
        if not (want_d or want_s):
            return None, None, None, dE, None, None, None, None
        dd = _f32(Gz.device, M, Np) if want_d else None
        ds = _f32(Gz.device, K, Np) if want_s else None
        if _any_elements(dd, ds):
            ent, stream = _kept_pattern_entry(ctx, crow, col, val)
            # (a copy when Gz has zero strides, e.g. after .sum(), or N % 8 != 0; bf16: read as it lies, a copy stays bf16)
            Grm, ldg = _rowmajor_ld(Gz, nnz, N, Np, torch.bfloat16 if ctx.bf16 else torch.float32)
            mul = op == api.EDGEOP_MUL                             # the only op whose gradients read an operand: the OTHER endpoint
            drm, ldd = _rowmajor_ld(x_dst if mul and want_s else None, M, N, Np)
            srm, lds = _rowmajor_ld(x_src if mul and want_d else None, K, N, Np)
            call = ent.eng.edge_op_backward_device_rm_bf16 if ctx.bf16 else ent.eng.edge_op_backward_device_rm
            call(op, Np, _ptr_nonempty(drm), ldd, _ptr_nonempty(srm), lds, _ptr_nonempty(Grm), ldg, _ptr_nonempty(dd), Np, _ptr_nonempty(ds), Np,
                 stream)
        return None, _cut_grad(dd, N, x_dst, want_d), _cut_grad(ds, N, x_src, want_s), dE, None, None, None, None


def _check_operands(A, x_dst, x_src, E, op):
    """The misuse edge_op() refuses, as vector_attention._check_operands does."""
    name = "edge_op"
    _check_sparse(A, name)
    if x_dst is None and op != "src":
        raise ValueError(name + ": op='" + op + "' reads x_dst")
    if x_src is None and op != "dst":
        raise ValueError(name + ": op='" + op + "' reads x_src")
    given = [t for t in (x_dst, x_src, E) if t is not None]
    if not all(isinstance(t, torch.Tensor) and t.layout == torch.strided and t.is_cuda for t in given):
        raise TypeError(name + " expects CUDA/HIP dense x_dst, x_src and E")
    first = given[0]
    if first.dim() < 2 or any(t.dim() != first.dim() or t.shape[1:] != first.shape[1:] for t in given):
        raise ValueError(name + ": x_dst is (M, N), x_src (K, N), E (nnz, N), with one trailing shape")
    if ((x_dst is not None and x_dst.shape[0] != A.shape[0]) or (x_src is not None and x_src.shape[0] != A.shape[1]) or
            (E is not None and E.shape[0] != A.values().numel()) or 0 in first.shape[1:]):
        raise ValueError("shape mismatch")


def edge_op(A, x_dst=None, x_src=None, E=None, op="add", fast=False):
    """One value per stored entry from both of its endpoints (DGL's u_add_v, u_sub_v, u_mul_v, copy_u and copy_v with the optional + e;
    the gSDDMM half next to the aggregations): for every stored entry e = (r, c) of A, in A's CSR entry order,
        op="add"  Z[e] = x_dst[r] + x_src[c]      (GatedGCN's pre-activations without the aggregation)
        op="sub"  Z[e] = x_dst[r] - x_src[c]      (Point Transformer's phi(x_i) - psi(x_j) + delta_ij with E; EdgeConv's x_j - x_i negated)
        op="mul"  Z[e] = x_dst[r] * x_src[c]      (the argument of an MLP on x_i * x_j)
        op="dst"  Z[e] = x_dst[r]                 op="src"  Z[e] = x_src[c]      (the halves of concat(e, x_i, x_j); x[rows], x[cols])
    plus E[e] when E is given -- every element one rounded fp32 operation and, with E, a second rounded add: the bits of the torch
    expression x_dst[rows] (op) x_src[cols] + E.  A is an (M, K) sparse_csr matrix of which only the PATTERN is used (its values are not
    read, the cached engine is not refreshed and A gets no gradient); x_dst is (M, N), x_src (K, N), E (nnz, N) in A's CSR entry order
    (torch_op.from_edge_index() gives the permutation for an edge list, torch_op.entry_rows() the row of every entry); all may carry any
    trailing shape instead of N, the same for all, which the result (nnz, ...) has too; fp32.  The operand an op does not read may be None
    (it is ignored otherwise); x_dst is x_src is fine on a square pattern.  One kernel pass (sextans_edge_op_device_rm): no gathered
    copies, no index tensors of 8 bytes per entry.  Differentiable in x_dst, x_src and E: E's gradient is the upstream gradient itself
    (no copy), the endpoints' are sums over A's rows and over A^T's rows (sextans_edge_op_backward_device_rm) in an order fixed by the
    pattern -- no atomics, the same bits on every run --, and only the passes whose gradients autograd wants are launched; not twice
    differentiable.  An N that is not a multiple of 8, and operands the kernel cannot read where they lie, are copied with zero padding,
    as gated.spmm_gated() does; `fast` only selects the cached engine.  The same op with the (nnz, N) tensors in bf16:
    sextans_amd.edge_op_bf16.edge_op_bf16()."""
    return _edge_op(A, x_dst, x_src, E, op, fast, False)


def _edge_op(A, x_dst, x_src, E, op, fast, bf16):
    """edge_op() (bf16 False) and edge_op_bf16.edge_op_bf16() (True): the checks, the reshapes and the call, once"""
    if not isinstance(op, str) or op not in _OPS:
        raise ValueError("op must be 'add', 'sub', 'mul', 'dst' or 'src'")
    code = _OPS[op]
    if op == "src":   # the operand an op does not read is ignored, whatever it is
        x_dst = None
    if op == "dst":
        x_src = None
    _check_operands(A, x_dst, x_src, E, op)
    M, K = A.shape
    first = x_dst if x_dst is not None else x_src
    tail = tuple(first.shape[1:])
    N = math.prod(tail)
    d2 = x_dst.reshape(M, N) if x_dst is not None else None
    s2 = d2 if x_src is x_dst else x_src.reshape(K, N) if x_src is not None else None
    E2 = E.reshape(E.shape[0], N) if E is not None else None
    if bf16 and E2 is not None and (E2.dtype != torch.bfloat16 or (N % 8 == 0 and not _qualifies(E2, N, N, torch.bfloat16))):
        raise ValueError("edge_op_bf16 takes E=None or a bf16 E that is row-major and 16-byte aligned "
                         "(one dtype for all (nnz, N) tensors of a call)")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (d2, s2, E2)):
        Z = _EdgeOpFunction.apply(A, d2, s2, E2, code, N, bool(fast), bf16)
    else:
        Z = _cut(_edge_op_forward(A, d2, s2, E2, code, N, bool(fast), bf16), N)
    return Z.reshape((Z.shape[0],) + tail)
