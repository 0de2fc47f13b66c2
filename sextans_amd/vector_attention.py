"""Channel-wise ("vector") attention from per-channel scores for torch: PointTransformerConv's
x_i' = sum_j softmax_j(gamma(phi(x_i) - psi(x_j) + delta_ij)) * (W x_j + delta_ij), DGL's edge_softmax on multi-channel edge data followed
by u_mul_e_sum / e_mul_e, PyG's softmax(alpha, index) with a per-channel alpha, as one fused pass over a sparse_csr pattern per direction.
Public: vector_attention().  The other ops of the torch front end live in sextans_amd.torch_op; this one shares their cached engines
(torch_op.cache_info() / clear_cache() cover it) and the frame of the tiled families in _op_aggregate.py."""
import math

import torch
from torch.autograd.function import once_differentiable

from . import api
from ._op_aggregate import _any_elements, _edge_bf16, _rowmajor_ld, _tiled_entry
from ._op_cache import _check_sparse, _cut, _cut_grad, _f32, _index_tensors, _keep_pattern, _kept_pattern_entry, _ptr_nonempty

__all__ = ["vector_attention"]


def _mode(V, D):
    return api.VATT_NODE if D is None else api.VATT_EDGE if V is None else api.VATT_ADD


def _edges_bf16(S, D, N):
    """do the edge tensors of a call go to the bf16 entry points as they lie: EVERY one that is given -- S, and D if present -- is bf16,
    N % 8 == 0, row-major, aligned (one dtype per call: a mixed or non-qualifying call takes the fp32 copies)"""
    return _edge_bf16(S, N) and (D is None or _edge_bf16(D, N))


def _vector_attention_forward(A, S, V, D, fast, want_lse):
    """(C, lse) of the engine's vector attention: (M, Np) with N padded up to a multiple of 8 (zero columns of S, V and D, which are cut
    again), lse None unless asked for.  V is None for VATT_EDGE, D for VATT_NODE.  bf16 S and D that the kernel can read where they lie
    go to the bf16 entry point as they are: the same bits, no fp32 copy of either."""
    nnz, N = S.shape
    M, K, Np, ent, stream, _ = _tiled_entry(A, N, fast)
    bf16 = _edges_bf16(S, D, N)
    e_dtype = torch.bfloat16 if bf16 else torch.float32
    Srm, lds = _rowmajor_ld(S, nnz, N, Np, e_dtype)
    Vrm, ldv = _rowmajor_ld(V, K, N, Np)
    Drm, ldd = _rowmajor_ld(D, nnz, N, Np, e_dtype)
    C = _f32(A.device, M, Np)
    lse = _f32(A.device, M, Np) if want_lse else None
    if _any_elements(C):
        call = ent.eng.vector_attention_device_rm_bf16 if bf16 else ent.eng.vector_attention_device_rm
        call(_mode(V, D), Np, _ptr_nonempty(Srm), lds, _ptr_nonempty(Vrm), ldv, _ptr_nonempty(Drm), ldd, _ptr_nonempty(C), Np,
             _ptr_nonempty(lse), Np, stream)
    return C, lse


class _VectorAttentionFunction(torch.autograd.Function):
    """vector_attention(): ONE forward call (sextans_vector_attention_device_rm) that keeps C and the log-sum-exp of every (row, column),
    ONE backward call (sextans_vector_attention_backward_device_rm) for the gradients that are wanted: a row pass that stores dS and dD,
    a column pass over A^T for dV.  A's values never enter: no gradient for A, no value refresh.  Not twice differentiable.
    bf16 S and D that went to the bf16 forward as they lie go to sextans_vector_attention_backward_device_rm_bf16 the same way, and the
    kernel writes dS and dD in bf16: the bits of the fp32 gradients rounded to their dtype, without the fp32 tensors."""

    @staticmethod
    def forward(ctx, A, S, V, D, fast):
        N = S.shape[1]
        C, lse = _vector_attention_forward(A, S, V, D, fast, True)
        ctx.save_for_backward(*_index_tensors(A), A.values(), S, V, D, C, lse)
        _keep_pattern(ctx, A, fast)
        out_lse = _cut(lse, N)
        ctx.mark_non_differentiable(out_lse)
        return _cut(C, N), out_lse

    @staticmethod
    @once_differentiable
    def backward(ctx, G, _):
        crow, col, val, S, V, D, C, lse = ctx.saved_tensors
        M, K = ctx.shape
        nnz, N = S.shape
        Np = C.shape[1]
        want_s = ctx.needs_input_grad[1]
        want_v = V is not None and ctx.needs_input_grad[2]
        want_d = D is not None and ctx.needs_input_grad[3]
        if not (want_s or want_v or want_d):
            return (None,) * 5
        ent, stream = _kept_pattern_entry(ctx, crow, col, val)
        Grm, ldg = _rowmajor_ld(G, M, N, Np)               # (a copy when G has zero strides, e.g. after .sum(), or N % 8 != 0)
        bf16 = _edges_bf16(S, D, N)                        # (the forward's route: one dtype for S, D, dS and dD)
        e_dtype = torch.bfloat16 if bf16 else torch.float32
        Srm, lds = _rowmajor_ld(S, nnz, N, Np, e_dtype)
        Vrm, ldv = _rowmajor_ld(V, K, N, Np)
        Drm, ldd = _rowmajor_ld(D, nnz, N, Np, e_dtype)
        dS = torch.empty((nnz, Np), dtype=e_dtype, device=G.device) if want_s else None
        dV = _f32(G.device, K, Np) if want_v else None
        dD = torch.empty((nnz, Np), dtype=e_dtype, device=G.device) if want_d else None
        if _any_elements(dS, dV, dD):
            call = ent.eng.vector_attention_backward_device_rm_bf16 if bf16 else ent.eng.vector_attention_backward_device_rm
            call(_mode(V, D), Np, _ptr_nonempty(Srm), lds, _ptr_nonempty(Vrm), ldv, _ptr_nonempty(Drm), ldd, _ptr_nonempty(C), Np,
                 _ptr_nonempty(lse), Np, _ptr_nonempty(Grm), ldg, _ptr_nonempty(dS), Np, _ptr_nonempty(dV), Np, _ptr_nonempty(dD), Np, stream)
        return None, _cut_grad(dS, N, S), _cut_grad(dV, N, V, want_v), _cut_grad(dD, N, D, want_d), None


def _check_operands(A, S, V, D):
    """The misuse vector_attention() refuses, as _op_aggregate._check_edge_operands does for the edge-feature ops."""
    name = "vector_attention"
    _check_sparse(A, name)
    if V is None and D is None:
        raise ValueError(name + ": V, D or both must be given")
    given = [t for t in (S, V, D) if t is not None]
    if not all(isinstance(t, torch.Tensor) and t.layout == torch.strided and t.is_cuda for t in given):
        raise TypeError(name + " expects CUDA/HIP dense S, V and D")
    if S.dim() < 2 or any(t.dim() != S.dim() or t.shape[1:] != S.shape[1:] for t in given):
        raise ValueError(name + ": S is (nnz, N), V (K, N), D (nnz, N), with one trailing shape")
    if (S.shape[0] != A.values().numel() or (V is not None and V.shape[0] != A.shape[1]) or (D is not None and D.shape[0] != S.shape[0]) or
            0 in S.shape[1:]):
        raise ValueError("shape mismatch")


def vector_attention(A, S, V=None, D=None, return_lse=False, fast=False):
    """Channel-wise attention from per-channel scores (Point Transformer's "vector attention"; DGL's edge_softmax on multi-channel edge
    data followed by u_mul_e_sum / e_mul_e; PyG's softmax(alpha, index) with a per-channel alpha in front of propagate):
        C[r, n] = sum over row r's stored entries e = (r, c) of softmax_e(S[e, n]) * m_e[n]
      V given, D None    m_e = V[c, :]              (plain vector attention)
      V and D given      m_e = V[c, :] + D[e, :]    (PointTransformerConv: value plus positional encoding, one rounded add)
      V None, D given    m_e = D[e, :]              (any message computed by the caller)
    -- a softmax per output channel over the row's scores, which are READ from S, a tensor of their own (the output of an MLP, say), not
    computed from the message.  A is an (M, K) sparse_csr matrix of which only the PATTERN is used (its values are not read, the cached
    engine is not refreshed and A gets no gradient); S and D are (nnz, N) IN A'S CSR ENTRY ORDER (torch_op.from_edge_index() gives the
    permutation for an edge list, torch_op.entry_rows() the row of every entry), V is (K, N); all three may carry any trailing shape
    instead of N, the same for all, which the result (M, ...) has too; fp32.  A score of -inf masks its (entry, channel): weight 0,
    gradient 0; a (row, channel) whose scores are all -inf gives NaN there; a row without entries gives 0.  One kernel pass per direction
    (sextans_vector_attention_device_rm / _backward_device_rm): online softmax, nothing of size nnz x N besides S, D and their gradients,
    no atomics -- the same bits on every run.  Differentiable in S, V and D; only the gradients asked for are computed (a row pass for
    dS and dD, a column pass over A^T for dV); not twice differentiable.  return_lse=True: also the (M, ...) log-sum-exp of the scores
    (-inf in an empty row; not differentiable).  An N that is not a multiple of 8, and operands the kernel cannot read where they lie,
    are copied with zero padding, as torch_op.spmm_edge() does; `fast` only selects the cached engine.  bf16 S and D (autocast) with
    N % 8 == 0 that are row-major and 16-byte aligned -- every edge tensor that is given, S alone in the first form -- are read as they
    lie and their gradients written in bf16 by the kernel (sextans_vector_attention_device_rm_bf16 / _backward_device_rm_bf16): the
    bits of the fp32 route, without an fp32 (nnz, N) tensor; C and lse stay fp32.  A mixed call (a bf16 S with an fp32 D, say) takes
    the fp32 copies as before."""
    _check_operands(A, S, V, D)
    M, K = A.shape
    tail = tuple(S.shape[1:])
    N = math.prod(tail)
    S2 = S.reshape(S.shape[0], N)
    V2 = V.reshape(K, N) if V is not None else None
    D2 = D.reshape(D.shape[0], N) if D is not None else None
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (S2, V2, D2)):
        C, lse = _VectorAttentionFunction.apply(A, S2, V2, D2, bool(fast))
    else:
        C, lse = (_cut(x, N) for x in _vector_attention_forward(A, S2, V2, D2, bool(fast), bool(return_lse)))
    C = C.reshape((M,) + tail)
    return (C, lse.reshape((M,) + tail)) if return_lse else C
