"""Softmax aggregation of edge-feature messages for torch: GENConv / DeeperGCN on graphs with edge features (message
relu(x_j + e_ij) + eps under a learnable-temperature softmax) and PyG's SoftmaxAggregation over any materialised message, as one fused pass
over a sparse_csr pattern per direction.  Public: spmm_edge_softagg().  The other ops of the torch front end live in sextans_amd.torch_op;
this one shares their cached engines (torch_op.cache_info() / clear_cache() cover it) and the frame of the tiled families in
_op_aggregate.py."""
import torch
from torch.autograd.function import once_differentiable

from . import api
from ._op_aggregate import _EDGE_OPS, _any_elements, _check_edge_operands, _edge_bf16, _rowmajor_ld, _tiled_entry
from ._op_cache import _cut, _cut_grad, _f32, _index_tensors, _keep_pattern, _kept_pattern_entry, _ptr, _ptr_nonempty

__all__ = ["spmm_edge_softagg"]


def _edge_softagg_forward(A, B, E, t, op, fast, want_lse):
    """(C, lse, tp) of the engine's edge-feature softmax aggregation: C and lse (M, Np) with N padded up to a multiple of 8 (zero columns
    of B and E), lse None unless asked for; tp the (Np,) fp32 temperatures handed to the kernel (padded columns: 1), None for t = 1
    everywhere.  B is None for EDGE_COPY.  A bf16 E that the kernel can read where it lies goes to the bf16 entry point as it is: the same
    bits, no fp32 copy of E."""
    nnz, N = E.shape
    M, K, Np, ent, stream, _ = _tiled_entry(A, N, fast)
    bf16 = _edge_bf16(E, N)
    Brm, ldb = _rowmajor_ld(B, K, N, Np)
    Erm, lde = _rowmajor_ld(E, nnz, N, Np, torch.bfloat16 if bf16 else torch.float32)
    tp = None
    if t is not None:
        tp = torch.ones((Np,), dtype=torch.float32, device=A.device)
        tp[:N] = t.detach()
    C = _f32(A.device, M, Np)
    lse = _f32(A.device, M, Np) if want_lse else None
    if _any_elements(C):
        call = ent.eng.spmm_edge_softagg_device_rm_bf16 if bf16 else ent.eng.spmm_edge_softagg_device_rm
        call(op, Np, _ptr_nonempty(Brm), ldb, _ptr_nonempty(Erm), lde, _ptr(tp), _ptr_nonempty(C), Np, _ptr_nonempty(lse), Np, stream)
    return C, lse, tp


class _SpmmEdgeSoftaggFunction(torch.autograd.Function):
    """spmm_edge_softagg(): ONE forward call (sextans_spmm_edge_softagg_device_rm) that keeps C and the log-sum-exp of every (row, column),
    ONE backward call (sextans_spmm_edge_softagg_backward_device_rm) for the gradients that are wanted: a column pass over A^T for dB, a
    row pass that stores dE and the rows' share of dt, the fixed-order sum over the rows for dt.  t is the (N,) tensor or None (= 1, no
    gradient); the workspace exists only when t wants a gradient.  A's values never enter: no gradient for A, no value refresh.  Not twice
    differentiable.  A bf16 E that went to the bf16 forward as it lies goes to sextans_spmm_edge_softagg_backward_device_rm_bf16 the same
    way, and the kernel writes dE in bf16: the bits of the fp32 dE rounded to E's dtype, without the fp32 tensors."""

    @staticmethod
    def forward(ctx, A, B, E, t, op, fast):
        N = E.shape[1]
        C, lse, tp = _edge_softagg_forward(A, B, E, t, op, fast, True)
        ctx.save_for_backward(*_index_tensors(A), A.values(), B, E, C, lse, tp)
        _keep_pattern(ctx, A, fast)
        ctx.op = op
        ctx.t_dtype = t.dtype if t is not None else None
        out_lse = _cut(lse, N)
        ctx.mark_non_differentiable(out_lse)
        return _cut(C, N), out_lse

    @staticmethod
    @once_differentiable
    def backward(ctx, G, _):
        crow, col, val, B, E, C, lse, tp = ctx.saved_tensors
        M, K = ctx.shape
        nnz, N = E.shape
        Np = C.shape[1]
        want_b, want_e = B is not None and ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        want_t = tp is not None and ctx.needs_input_grad[3]
        if not (want_b or want_e or want_t):
            return (None,) * 6
        ent, stream = _kept_pattern_entry(ctx, crow, col, val)
        Grm, ldg = _rowmajor_ld(G, M, N, Np)               # (a copy when G has zero strides, e.g. after .sum(), or N % 8 != 0)
        Brm, ldb = _rowmajor_ld(B, K, N, Np)
        bf16 = _edge_bf16(E, N)                            # (the forward's route: one dtype for E and dE)
        e_dtype = torch.bfloat16 if bf16 else torch.float32
        Erm, lde = _rowmajor_ld(E, nnz, N, Np, e_dtype)
        dB = _f32(G.device, K, Np) if want_b else None
        dE = torch.empty((nnz, Np), dtype=e_dtype, device=G.device) if want_e else None
        dt = _f32(G.device, Np) if want_t else None
        work = _f32(G.device, max(ent.eng.spmm_edge_softagg_workspace_floats(Np), 1)) if want_t else None
        if _any_elements(dB, dE, dt):
            call = ent.eng.spmm_edge_softagg_backward_device_rm_bf16 if bf16 else ent.eng.spmm_edge_softagg_backward_device_rm
            call(ctx.op, Np, _ptr_nonempty(Brm), ldb, _ptr_nonempty(Erm), lde, _ptr_nonempty(tp), _ptr_nonempty(C), Np, _ptr_nonempty(lse), Np,
                 _ptr_nonempty(Grm), ldg, _ptr_nonempty(dB), Np, _ptr_nonempty(dE), Np, _ptr_nonempty(dt), _ptr_nonempty(work), stream)
        gt = _cut(dt, N).to(ctx.t_dtype) if want_t else None
        return None, _cut_grad(dB, N, B), _cut_grad(dE, N, E), gt, None, None


def spmm_edge_softagg(A, B, E, op="mul", t=1.0, eps=0.0, return_lse=False, fast=False):
    """Softmax aggregation of messages with a feature vector per stored entry (GENConv / DeeperGCN with edge features; PyG's
    SoftmaxAggregation(t, learn=True) over a materialised message):
        C[r, n] = sum over row r's stored entries e = (r, c) of softmax_e(t[n] * m_e[n]) * m_e[n]   (+ eps on rows that have entries)
      op="mul"       m_e = B[c, :] * E[e, :]
      op="add"       m_e = B[c, :] + E[e, :]
      op="add_relu"  m_e = relu(B[c, :] + E[e, :])      (GENConv: relu(x_j + e_ij); its "+ eps" is the eps argument)
      op="copy"      m_e = E[e, :], B=None              (any message computed by the caller)
    -- a softmax per output column over the row's messages themselves (one rounded fp32 operation each).  A is an (M, K) sparse_csr
    matrix of which only the PATTERN is used (its values are not read, the cached engine is not refreshed and A gets no gradient); B is
    (K, N), E is (nnz, N) IN A'S CSR ENTRY ORDER (torch_op.from_edge_index() gives the permutation for an edge list); the result is a
    dense fp32 (M, N) tensor.  t is the temperature: a Python float, a 0-d tensor or an (N,) tensor, any finite values; 0 gives the
    mean, large values the max, negative ones a soft minimum.  A shift common to a row's messages cancels in the softmax weights, so
    GENConv's message relu(x_j + e_ij) + eps aggregates to C + eps: eps is added to the rows that have entries; a row without entries
    gives 0.  One kernel pass per direction (sextans_spmm_edge_softagg_device_rm / _backward_device_rm): online softmax, nothing of size
    nnz x N besides E and its gradient, no atomics -- the same bits on every run.  Differentiable in B, E and in t when it is a tensor
    that requires grad (a 0-d t gets the sum over the columns); only the gradients asked for are computed; they lose digits where
    |t (m - C)| is large.  return_lse=True: also the (M, N) log-sum-exp of the scores t m (-inf in an empty row; not differentiable; of
    the messages without eps).  An N that is not a multiple of 8, and operands the kernel cannot read where they lie, are copied with
    zero padding, as torch_op.spmm_edge() does; `fast` only selects the cached engine.  A bf16 E (autocast) with N % 8 == 0 that is
    row-major and 16-byte aligned is read as it lies and its gradient written in bf16 by the kernel
    (sextans_spmm_edge_softagg_device_rm_bf16 / _backward_device_rm_bf16): the bits of the fp32 route, without an fp32 (nnz, N) tensor;
    C and lse stay fp32."""
    _check_edge_operands(A, B, E, op, "spmm_edge_softagg")
    N = E.shape[1]
    if isinstance(t, torch.Tensor):
        if t.dim() > 1 or (t.dim() == 1 and t.shape[0] != N):
            raise ValueError("t must be a float, a 0-d tensor or an (N,) tensor")
        if not t.is_floating_point():
            raise TypeError("t must be a floating-point tensor")
        tv = t.to(E.device).expand(N)   # (autograd sums a scalar's gradient back)
    elif float(t) == 1.0:
        tv = None                       # the kernels' t == NULL path
    else:
        tv = torch.full((N,), float(t), dtype=torch.float32, device=E.device)
    code = _EDGE_OPS[op]
    if torch.is_grad_enabled() and ((B is not None and B.requires_grad) or E.requires_grad or (tv is not None and tv.requires_grad)):
        C, lse = _SpmmEdgeSoftaggFunction.apply(A, B, E, tv, code, bool(fast))
    else:
        C, lse = (_cut(x, N) for x in _edge_softagg_forward(A, B, E, tv, code, bool(fast), bool(return_lse))[:2])
    eps = float(eps)
    if eps != 0.0:
        crow = _index_tensors(A)[0]
        C = C + eps * (crow[1:] > crow[:-1]).to(C.dtype)[:, None]
    return (C, lse) if return_lse else C
