"""The attention ops of the torch front end (private; sextans_amd.torch_op is the public import point): the fused attention, the one with
edge features, GAT, GATv2 and the attention from caller-supplied scores, their dropout, and the composition of the product ops.

The five fused families share one frame, written once in the helpers below; their Functions state what differs: the operands (per-head
vectors through _heads_operand, per-head scalars through _scalars_operand), the engine entry with its argument list, and the gradient
buffers.  Every family calls the engine's *_dropout_* entry with a sextans_dropout that is NULL when nothing is dropped: the C ABI
documents that as the entry without dropout, so the choice is made in _drop_struct alone."""
import functools
import math

import torch
from torch.autograd.function import once_differentiable

from . import api
from ._op_cache import (_carry, _check_dense, _check_sparse, _cut, _cut_grad, _f32, _grad_values, _index_tensors, _keep_pattern,
                        _kept_pattern_entry, _pattern_entry_of, _pattern_grad, _ptr, _vals32)
from ._op_product import row_softmax, sddmm, spmm


# --- the frame of the fused families ---------------------------------------------------------------------------------------------------
def _pad8(d):
    """a head dimension as the kernels take it: the next multiple of 8 (_cut / _cut_grad are the way back)"""
    return -(-d // 8) * 8


def _heads_operand(t, dp):
    """A (rows, H, d) tensor as the fused kernels read it: t itself where it lies that way (fp32, heads side by side in a row, d % 8 == 0,
    16-byte aligned base and row stride), else a zero-padded contiguous fp32 copy (rows, H, dp)."""
    rows, H, d = t.shape
    if (t.dtype == torch.float32 and d == dp and t.stride(2) == 1 and (H == 1 or t.stride(1) == d) and t.stride(0) >= H * d and
            t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0):
        return t, t.stride(0)
    out = torch.zeros((rows, H, dp), dtype=torch.float32, device=t.device)
    out[:, :, :d] = t
    return out, H * dp


def _scalars_operand(t):
    """A (rows, H) tensor of per-node, per-head scalars as the GAT kernels read it: t itself where it lies that way (fp32, the heads of a
    row next to each other, rows at least H apart, 16-byte aligned base), else a contiguous fp32 copy."""
    rows, H = t.shape
    if t.dtype == torch.float32 and (H == 1 or t.stride(1) == 1) and t.stride(0) >= H and t.data_ptr() % 16 == 0:
        return t, t.stride(0)
    out = torch.empty((rows, H), dtype=torch.float32, device=t.device)
    out.copy_(t)
    return out, H


def _bias_operands(val, bias, want_grad=False):
    """A's values as the kernels' additive bias -> (the fp32 vector, None without bias; the buffer of its gradient, None unless wanted).
    _pattern_grad() makes A's gradient of the latter."""
    return (_vals32(val) if bias else None), (_f32(val.device, val.numel()) if bias and want_grad else None)


def _out_buffers(device, M, H, dvp, lse=True):
    """-> (O (M, H, dvp), the rows' log-sum-exp (M, H) -- empty for a family mode that has none)"""
    return _f32(device, M, H, dvp), _f32(device, *((M, H) if lse else (0,)))


def _check_dropout(p):
    p = float(p)
    if not (0.0 <= p < 1.0):
        raise ValueError("dropout must be in [0, 1)")
    return p


def _draw_seed(seed):
    """seed=None: one int64 from torch's default CPU generator, so torch.manual_seed reproduces a run"""
    return int(torch.empty((), dtype=torch.int64).random_()) if seed is None else int(seed)


def _check_step(step, device):
    if step is None:
        return None
    if not (isinstance(step, torch.Tensor) and step.is_cuda and step.numel() == 1 and step.dtype in (torch.int64, torch.uint64) and
            step.device == device):
        raise TypeError("step must be None or a one-element int64 / uint64 tensor on A's device")
    return step


def _dropout_args(p, seed, step, device):
    """(checked dropout, seed, step) of a public call as the Functions take them: with dropout one seed is drawn (if None) and step is
    validated, in that order; without, (0.0, 0, None) -- no seed is drawn, torch's generator does not move, step is not looked at."""
    if p > 0.0:
        return p, _draw_seed(seed), _check_step(step, device)
    return 0.0, 0, None


def _drop_struct(p, seed, step):
    """The engine's view of (dropout, seed, step): None when nothing is dropped (the *_dropout_* entries are then the ones without)"""
    return api.Dropout(p, seed, _ptr(step)) if p > 0.0 else None


def _with_heads(t, rank):
    """an operand given without its heads dimension (one head) in the rank the Functions take"""
    return t if t.dim() == rank else t.unsqueeze(1)


def _result_like(out, t):
    """the (rows, H, d) result in the rank of the operand t that decides it"""
    return out if t.dim() == 3 else out[:, 0]


def _check_slope(negative_slope):
    slope = float(negative_slope)
    if not (slope >= 0.0) or math.isinf(slope):
        raise ValueError("negative_slope must be finite and >= 0")
    return slope


# --- dropout mask and the composition ------------------------------------------------------------------------------------------------
def dropout_mask(A, heads, p, seed, step=None):
    """The attention-dropout multipliers the fused kernels apply (sextans_dropout_mask_device): an (nnz, heads) fp32 tensor on A's
    device, 1 / (1 - p) where (entry, head) is kept, 0 where it is dropped; entries in A's CSR order.  step: None (0), or a one-element
    int64 / uint64 tensor on the device whose value is added to the seed when the kernel runs."""
    _check_sparse(A, "dropout_mask")
    p = _check_dropout(p)
    heads = int(heads)
    if heads < 1:
        raise ValueError("heads must be >= 1")
    step = _check_step(step, A.device)
    ent, stream, _, _, val = _pattern_entry_of(A, False)
    out = torch.empty((val.numel(), heads), dtype=torch.float32, device=A.device)
    if out.numel():
        ent.eng.dropout_mask_device(heads, api.Dropout(p, int(seed), _ptr(step)), out.data_ptr(), stream)
    return out


class _ScaleValuesFunction(torch.autograd.Function):
    """P with its values multiplied by a constant vector (one head's column of dropout_mask): the composition's dropout.  The gradient
    is the upstream gradient's values times the same vector."""

    @staticmethod
    def forward(ctx, P, mult):
        crow, col = _index_tensors(P)
        ctx.save_for_backward(crow, col, mult)
        ctx.shape, ctx.vdtype = tuple(P.shape), P.values().dtype
        return torch.sparse_csr_tensor(crow, col, (P.values().detach().to(torch.float32) * mult).to(ctx.vdtype), size=ctx.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        crow, col, mult = ctx.saved_tensors
        g = _grad_values(G, crow, col, int(mult.numel()))
        return torch.sparse_csr_tensor(crow, col, (g * mult).to(ctx.vdtype), size=ctx.shape), None


def _composed_attention(A, Q, K, V, scale, bias, fast, mult):
    """one head of the composition; mult: None, or the head's column of dropout_mask()"""
    S = sddmm(A, Q, K, 1.0, 1.0 if bias else 0.0, fast)
    P = row_softmax(S, scale, fast)
    if mult is not None:
        crow, col = _index_tensors(P)
        P = _carry(_ScaleValuesFunction.apply(P, mult), crow, col)
    return spmm(P, V, fast=fast)


# --- fused attention -----------------------------------------------------------------------------------------------------------------
class _FusedAttentionFunction(torch.autograd.Function):
    """sparse_attention(fused=True): one kernel pass forward (sextans_attention_device), a row pass and a column pass backward
    (sextans_attention_backward_device), all heads at once.  Nothing of size nnz is kept: the backward recomputes the probabilities from
    the rows' log-sum-exp.  A's values enter as an explicit bias pointer, never through the engine: no value refresh anywhere."""

    @staticmethod
    def forward(ctx, A, Q, K, V, scale, bias, fast, p=0.0, seed=0, step=None):
        M, Kk = A.shape
        H, d, dv = Q.shape[1], Q.shape[2], V.shape[2]
        dp, dvp = _pad8(d), _pad8(dv)
        ent, stream, crow, col, val = _pattern_entry_of(A, fast)
        Qr, ldq = _heads_operand(Q.detach(), dp)
        Kr, ldk = _heads_operand(K.detach(), dp)
        Vr, ldv = _heads_operand(V.detach(), dvp)
        b, _ = _bias_operands(val, bias)
        O, lse = _out_buffers(A.device, M, H, dvp)
        ent.eng.attention_dropout_device(H, dp, dvp, scale, Qr.data_ptr(), ldq, Kr.data_ptr(), ldk, Vr.data_ptr(), ldv, _ptr(b),
                                         O.data_ptr(), H * dvp, lse.data_ptr(), _drop_struct(p, seed, step), stream)
        ctx.save_for_backward(crow, col, val, Q, K, V, O, lse)
        _keep_pattern(ctx, A, fast)
        ctx.scale, ctx.bias = scale, bias
        ctx.drop = (p, seed, step)   # the backward recomputes the forward's mask
        return _cut(O, dv)

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        crow, col, val, Q, K, V, O, lse = ctx.saved_tensors
        M, Kk = ctx.shape
        H, d, dv = Q.shape[1], Q.shape[2], V.shape[2]
        dp, dvp = _pad8(d), O.shape[2]
        ent, stream = _kept_pattern_entry(ctx, crow, col, val)
        Qr, ldq = _heads_operand(Q.detach(), dp)
        Kr, ldk = _heads_operand(K.detach(), dp)
        Vr, ldv = _heads_operand(V.detach(), dvp)
        Gr, ldg = _heads_operand(G, dvp)           # (a copy when G has zero strides, e.g. after .sum(), or dv % 8 != 0)
        b, db = _bias_operands(val, ctx.bias, ctx.needs_input_grad[0])
        new = functools.partial(_f32, G.device)
        delta, dQ, dK, dV = new(M, H), new(M, H, dp), new(Kk, H, dp), new(Kk, H, dvp)
        ent.eng.attention_dropout_backward_device(H, dp, dvp, ctx.scale, Qr.data_ptr(), ldq, Kr.data_ptr(), ldk, Vr.data_ptr(), ldv, _ptr(b),
                                                  O.data_ptr(), H * dvp, lse.data_ptr(), Gr.data_ptr(), ldg, delta.data_ptr(),
                                                  dQ.data_ptr(), H * dp, dK.data_ptr(), H * dp, dV.data_ptr(), H * dvp, _ptr(db),
                                                  _drop_struct(*ctx.drop), stream)
        need = ctx.needs_input_grad
        return (_pattern_grad(crow, col, val, db, ctx.shape), _cut_grad(dQ, d, Q, need[1]), _cut_grad(dK, d, K, need[2]),
                _cut_grad(dV, dv, V, need[3]), None, None, None, None, None, None)


def sparse_attention(A, Q, K, V, scale=None, bias=False, fast=False, fused=False):
    """softmax(scale * (Q K^T [+ A]) restricted to A's pattern) V, per head.
    A (M x Kk) gives the pattern -- and, with bias=True, an additive bias / mask through its values, shared by all heads; Q is (M, d),
    K (Kk, d), V (Kk, dv), or with heads (M, H, d), (Kk, H, d), (Kk, H, dv); the result has V's rank.  scale=None means 1 / sqrt(d).
    Differentiable in Q, K, V and (bias=True) A.
    fused=False (default): spmm(row_softmax(sddmm(A, Q, K, beta=bias), scale), V), a composition of the three ops on one cached engine
    with S and P materialised (the backward needs P) and handed to the engine as value refreshes; with heads, once per head, the
    results stacked.
    fused=True: one kernel pass per direction for all heads (sextans_attention_device / sextans_attention_backward_device): online
    softmax, nothing of size nnz written, no value refresh; the backward keeps O and M * H floats instead of S and P.  Within the
    tolerance of a chain of fp32 operations of the composition, not bit-equal to it.  Head dimensions up to 128; those that are not
    multiples of 8, and operands that do not lie as the kernels read them, are copied with zero padding."""
    return _sparse_attention(A, Q, K, V, scale, bias, fast, fused, 0.0, 0, None)


def sparse_attention_dropout(A, Q, K, V, dropout, seed=None, step=None, scale=None, bias=False, fast=False, fused=False):
    """sparse_attention() with dropout on the normalised attention coefficients (attn_drop): every (entry, head) coefficient is zeroed
    with probability `dropout` and the others are multiplied by 1 / (1 - dropout), after the softmax (dropped entries still count in the
    row's sum).  dropout in [0, 1), else ValueError; 0 is sparse_attention() itself, bit for bit.
    The mask is a hash of (seed + step, entry, head), bit-reproducible.  seed=None draws one int64 from torch's default CPU generator, so
    torch.manual_seed reproduces a run; step: None, or a one-element int64 / uint64 tensor on the device that the kernels read when
    they run -- a captured graph draws a new mask on every replay when the caller bumps it in between.  The backward uses the forward's
    seed and step.
    fused=True: the mask is recomputed inside the kernels of all three passes (sextans_attention_dropout_device /
    sextans_attention_dropout_backward_device); nothing of size nnz exists.  fused=False: the composition with P multiplied by
    dropout_mask()'s column of the head before the SpMM -- the same mask, so both agree within the tolerance of sparse_attention()."""
    return _sparse_attention(A, Q, K, V, scale, bias, fast, fused, _check_dropout(dropout), seed, step)


def _check_qkv(A, Q, K, V):
    """Q, K and V of the attention with heads -> (Q3, K3, V3, H, d, dv)"""
    if any(t.dim() not in (2, 3) for t in (Q, K, V)):
        raise ValueError("Q, K and V are (rows, d) or (rows, heads, d)")
    Q3, K3, V3 = (_with_heads(t, 3) for t in (Q, K, V))
    M, Kk = A.shape
    H, d, dv = Q3.shape[1], Q3.shape[2], V3.shape[2]
    if K3.shape[1] != H or V3.shape[1] != H:
        raise ValueError("Q, K and V differ in their number of heads")
    if Q3.shape[0] != M or K3.shape[0] != Kk or V3.shape[0] != Kk or K3.shape[2] != d or H == 0 or d == 0 or dv == 0:
        raise ValueError("shape mismatch")
    return Q3, K3, V3, H, d, dv


def _sparse_attention(A, Q, K, V, scale, bias, fast, fused, p, seed, step):
    _check_sparse(A, "sparse_attention")
    _check_dense("sparse_attention", "Q, K and V", Q, K, V)
    if not fused and Q.dim() == 2 and K.dim() == 2 and V.dim() == 2:
        if V.shape[0] != A.shape[1]:
            raise ValueError("shape mismatch")
        if scale is None:
            scale = 1.0 / math.sqrt(Q.shape[1])
        mult = dropout_mask(A, 1, p, _draw_seed(seed), step)[:, 0] if p > 0.0 else None
        return _composed_attention(A, Q, K, V, scale, bias, fast, mult)
    Q3, K3, V3, H, d, dv = _check_qkv(A, Q, K, V)
    if scale is None:
        scale = 1.0 / math.sqrt(d)
    p, seed, step = _dropout_args(p, seed, step, A.device)
    if not fused:
        mult = dropout_mask(A, H, p, seed, step) if p > 0.0 else None
        out = torch.stack([_composed_attention(A, Q3[:, h], K3[:, h], V3[:, h], scale, bias, fast,
                                               mult[:, h].contiguous() if mult is not None else None) for h in range(H)], dim=1)
    else:
        if d > 128 or dv > 128:
            raise ValueError("fused sparse_attention: head dimensions up to 128")
        out = _FusedAttentionFunction.apply(A, Q3, K3, V3, float(scale), bool(bias), bool(fast), p, seed, step)
    return _result_like(out, V)


# --- attention with edge features ----------------------------------------------------------------------------------------------------
def _edge_operands(Ek, Ev, shared, H, dp, dvp):
    """the optional per-entry key and value rows as the kernels read them -> (Ekr, ldek, Evr, ldev); shared: Ev is Ek itself"""
    Ekr, ldek = _heads_operand(Ek.detach(), dp) if Ek is not None else (None, H * dp)
    Evr, ldev = (Ekr, ldek) if shared else _heads_operand(Ev.detach(), dvp) if Ev is not None else (None, H * dvp)
    return Ekr, ldek, Evr, ldev


class _EdgeAttentionFunction(torch.autograd.Function):
    """sparse_attention_edge(): the fused attention with a key row and a value row per stored entry (sextans_attention_edge_device /
    sextans_attention_edge_backward_device).  Ek / Ev: (nnz, H, d) / (nnz, H, dv) or None; shared: Ev is Ek itself -- the backward then
    hands one buffer to the engine as both gradients and gets their sum.  As _FusedAttentionFunction: nothing of size nnz but E, dE and
    the bias, no value refresh."""

    @staticmethod
    def forward(ctx, A, Q, K, V, Ek, Ev, shared, scale, bias, fast, p, seed, step):
        M, Kk = A.shape
        H, d, dv = Q.shape[1], Q.shape[2], V.shape[2]
        dp, dvp = _pad8(d), _pad8(dv)
        ent, stream, crow, col, val = _pattern_entry_of(A, fast)
        Qr, ldq = _heads_operand(Q.detach(), dp)
        Kr, ldk = _heads_operand(K.detach(), dp)
        Vr, ldv = _heads_operand(V.detach(), dvp)
        Ekr, ldek, Evr, ldev = _edge_operands(Ek, Ev, shared, H, dp, dvp)
        b, _ = _bias_operands(val, bias)
        O, lse = _out_buffers(A.device, M, H, dvp)
        ent.eng.attention_edge_device(H, dp, dvp, scale, Qr.data_ptr(), ldq, Kr.data_ptr(), ldk, Vr.data_ptr(), ldv, _ptr(Ekr), ldek,
                                      _ptr(Evr), ldev, _ptr(b), O.data_ptr(), H * dvp, lse.data_ptr(), _drop_struct(p, seed, step), stream)
        ctx.save_for_backward(crow, col, val, Q, K, V, Ek, Ev, O, lse)
        _keep_pattern(ctx, A, fast)
        ctx.scale, ctx.bias, ctx.shared = scale, bias, shared
        ctx.drop = (p, seed, step)   # the backward recomputes the forward's mask
        return _cut(O, dv)

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        crow, col, val, Q, K, V, Ek, Ev, O, lse = ctx.saved_tensors
        M, Kk = ctx.shape
        H, d, dv = Q.shape[1], Q.shape[2], V.shape[2]
        dp, dvp = _pad8(d), O.shape[2]
        nnz, shared, need = int(val.numel()), ctx.shared, ctx.needs_input_grad
        ent, stream = _kept_pattern_entry(ctx, crow, col, val)
        Qr, ldq = _heads_operand(Q.detach(), dp)
        Kr, ldk = _heads_operand(K.detach(), dp)
        Vr, ldv = _heads_operand(V.detach(), dvp)
        Ekr, ldek, Evr, ldev = _edge_operands(Ek, Ev, shared, H, dp, dvp)
        Gr, ldg = _heads_operand(G, dvp)
        b, db = _bias_operands(val, ctx.bias, need[0])
        new = functools.partial(_f32, G.device)
        delta, dQ, dK, dV = new(M, H), new(M, H, dp), new(Kk, H, dp), new(Kk, H, dvp)
        dEk = new(nnz, H, dp) if Ek is not None and need[4] else None
        dEv = dEk if shared else new(nnz, H, dvp) if Ev is not None and need[5] else None   # shared: ONE buffer, the sum
        ent.eng.attention_edge_backward_device(H, dp, dvp, ctx.scale, Qr.data_ptr(), ldq, Kr.data_ptr(), ldk, Vr.data_ptr(), ldv, _ptr(Ekr), ldek,
                                               _ptr(Evr), ldev, _ptr(b), O.data_ptr(), H * dvp, lse.data_ptr(), Gr.data_ptr(), ldg,
                                               delta.data_ptr(), dQ.data_ptr(), H * dp, dK.data_ptr(), H * dp, dV.data_ptr(), H * dvp,
                                               _ptr(dEk), H * dp, _ptr(dEv), H * dvp, _ptr(db), _drop_struct(*ctx.drop), stream)
        return (_pattern_grad(crow, col, val, db, ctx.shape), _cut_grad(dQ, d, Q, need[1]), _cut_grad(dK, d, K, need[2]),
                _cut_grad(dV, dv, V, need[3]), _cut_grad(dEk, d, Ek), _cut_grad(dEv, dv, Ev, not shared),
                None, None, None, None, None, None, None)


def sparse_attention_edge(A, Q, K, V, edge_key=None, edge_value=None, scale=None, bias=False, dropout=0.0, seed=None, step=None, fast=False):
    """Attention on A's pattern with a feature vector per stored entry inside it (TransformerConv(edge_dim=...), UniMP, relative-position
    encodings): for the entry e = (r, c) of row r and head h
        s_e = scale * (<Q[r, h], K[c, h] + edge_key[e, h]> + A_e if bias),   O[r, h] = sum_e softmax_e(s) (V[c, h] + edge_value[e, h])
    Always fused: one kernel pass forward, a row pass and a column pass backward (sextans_attention_edge_device /
    sextans_attention_edge_backward_device), all heads at once, the edge rows read where they lie.  Q is (M, d) or (M, H, d), K (Kk, d) /
    (Kk, H, d), V (Kk, dv) / (Kk, H, dv); edge_key is (nnz, H * d) or (nnz, H, d), edge_value (nnz, H * dv) or (nnz, H, dv), both in A's
    entry order (from_edge_index's perm brings a PyG edge_attr there); either may be None.  The result has V's rank.  scale=None means
    1 / sqrt(d); dropout, seed, step as sparse_attention_dropout().  Differentiable in Q, K, V, both edge tensors and (bias=True) A.
    edge_key is edge_value (one projected edge_attr for both sides, d == dv): the backward stores the sum of the two gradients once and
    returns it -- no second (nnz, H, d) buffer exists.  One cached engine per pattern, no value refresh."""
    _check_sparse(A, "sparse_attention_edge")
    _check_dense("sparse_attention_edge", "Q, K and V", Q, K, V)
    if any(t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda) for t in (edge_key, edge_value)):
        raise TypeError("sparse_attention_edge expects CUDA/HIP dense edge_key and edge_value (or None)")
    Q3, K3, V3, H, d, dv = _check_qkv(A, Q, K, V)
    if d > 128 or dv > 128:
        raise ValueError("sparse_attention_edge: head dimensions up to 128")
    nnz = int(A.values().numel())
    shared = edge_key is not None and edge_key is edge_value

    def edge3(t, w, name):
        if t is None:
            return None
        if t.dim() not in (2, 3) or t.shape[0] != nnz or (tuple(t.shape[1:]) != (H, w) if t.dim() == 3 else t.shape[1] != H * w):
            raise ValueError("%s is (nnz, heads * d) or (nnz, heads, d) in A's entry order" % name)
        return t if t.dim() == 3 else t.unflatten(1, (H, w))

    Ek3 = edge3(edge_key, d, "edge_key")
    Ev3 = None if shared else edge3(edge_value, dv, "edge_value")
    if shared and d != dv:
        raise ValueError("edge_key is edge_value needs d == dv")
    if scale is None:
        scale = 1.0 / math.sqrt(d)
    p, seed, step = _dropout_args(_check_dropout(dropout), seed, step, A.device)
    out = _EdgeAttentionFunction.apply(A, Q3, K3, V3, Ek3, Ev3, shared, float(scale), bool(bias), bool(fast), p, seed, step)
    return _result_like(out, V)


# --- GAT -----------------------------------------------------------------------------------------------------------------------------
class _GatAttentionFunction(torch.autograd.Function):
    """gat_attention(): one kernel pass forward (sextans_gat_attention_device), a row pass and a column pass backward
    (sextans_gat_attention_backward_device), all heads at once.  Nothing of size nnz is kept: the backward recomputes the scores and the
    probabilities from the rows' log-sum-exp.  A's values enter as an explicit bias pointer, never through the engine: no value refresh
    anywhere."""

    @staticmethod
    def forward(ctx, A, adst, asrc, V, slope, bias, fast, p=0.0, seed=0, step=None):
        M, Kk = A.shape
        H, dv = V.shape[1], V.shape[2]
        dvp = _pad8(dv)
        ent, stream, crow, col, val = _pattern_entry_of(A, fast)
        ad, ldad = _scalars_operand(adst.detach())
        as_, ldas = _scalars_operand(asrc.detach())
        Vr, ldv = _heads_operand(V.detach(), dvp)
        b, _ = _bias_operands(val, bias)
        O, lse = _out_buffers(A.device, M, H, dvp)
        ent.eng.gat_attention_dropout_device(H, dvp, slope, ad.data_ptr(), ldad, as_.data_ptr(), ldas, Vr.data_ptr(), ldv, _ptr(b),
                                             O.data_ptr(), H * dvp, lse.data_ptr(), _drop_struct(p, seed, step), stream)
        ctx.save_for_backward(crow, col, val, adst, asrc, V, O, lse)
        _keep_pattern(ctx, A, fast)
        ctx.slope, ctx.bias = slope, bias
        ctx.drop = (p, seed, step)   # the backward recomputes the forward's mask
        return _cut(O, dv)

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        crow, col, val, adst, asrc, V, O, lse = ctx.saved_tensors
        M, Kk = ctx.shape
        H, dv = V.shape[1], V.shape[2]
        dvp = O.shape[2]
        ent, stream = _kept_pattern_entry(ctx, crow, col, val)
        ad, ldad = _scalars_operand(adst.detach())
        as_, ldas = _scalars_operand(asrc.detach())
        Vr, ldv = _heads_operand(V.detach(), dvp)
        Gr, ldg = _heads_operand(G, dvp)           # (a copy when G has zero strides, e.g. after .sum(), or dv % 8 != 0)
        b, db = _bias_operands(val, ctx.bias, ctx.needs_input_grad[0])
        new = functools.partial(_f32, G.device)
        delta, dad, das, dV = new(M, H), new(M, H), new(Kk, H), new(Kk, H, dvp)
        ent.eng.gat_attention_dropout_backward_device(H, dvp, ctx.slope, ad.data_ptr(), ldad, as_.data_ptr(), ldas, Vr.data_ptr(), ldv, _ptr(b),
                                                      O.data_ptr(), H * dvp, lse.data_ptr(), Gr.data_ptr(), ldg, delta.data_ptr(),
                                                      dad.data_ptr(), H, das.data_ptr(), H, dV.data_ptr(), H * dvp, _ptr(db),
                                                      _drop_struct(*ctx.drop), stream)
        need = ctx.needs_input_grad
        return (_pattern_grad(crow, col, val, db, ctx.shape), _cut_grad(dad, H, adst, need[1]), _cut_grad(das, H, asrc, need[2]),
                _cut_grad(dV, dv, V, need[3]), None, None, None, None, None, None)


def gat_attention(A, a_dst, a_src, V, negative_slope=0.2, bias=False, fast=False):
    """Graph attention (GAT, as GATConv in PyG / DGL) on A's pattern, per head:
        softmax over row r's stored entries (r, c) of leaky_relu(a_dst[r] + a_src[c] [+ A_e], negative_slope), times V.
    A (M x Kk) gives the edges -- entry (r, c): source c, destination r -- and, with bias=True, an additive edge term / mask through its
    values, shared by all heads (-inf masks an edge for every slope).  a_dst is (M,) or (M, H), a_src (Kk,) or (Kk, H): the two halves
    of GAT's attention vector applied to the transformed node features; V is (Kk, dv) or (Kk, H, dv), the result has V's rank.
    One kernel pass per direction for all heads (sextans_gat_attention_device / sextans_gat_attention_backward_device): online softmax,
    nothing of size nnz written, no value refresh; the backward keeps O and M * H floats.  Differentiable in a_dst, a_src, V and
    (bias=True) A; gradients come in the operands' dtypes.  dv up to 128; a dv that is not a multiple of 8, and operands that do not lie
    as the kernels read them, are copied (V with zero padding).  negative_slope: finite, >= 0."""
    return _gat_attention(A, a_dst, a_src, V, negative_slope, bias, fast, 0.0, 0, None)


def gat_attention_dropout(A, a_dst, a_src, V, dropout, seed=None, step=None, negative_slope=0.2, bias=False, fast=False):
    """gat_attention() with dropout on the normalised attention coefficients, as GATConv(dropout=...) in PyG and attn_drop in DGL (the
    GAT paper trains with 0.6): made inside the fused kernels of all three passes (sextans_gat_attention_dropout_device /
    sextans_gat_attention_dropout_backward_device), nothing of size nnz exists.  dropout, seed and step as in
    sparse_attention_dropout(); dropout=0 is gat_attention() itself, bit for bit."""
    return _gat_attention(A, a_dst, a_src, V, negative_slope, bias, fast, _check_dropout(dropout), seed, step)


def _gat_attention(A, a_dst, a_src, V, negative_slope, bias, fast, p, seed, step):
    _check_sparse(A, "gat_attention")
    _check_dense("gat_attention", "a_dst, a_src and V", a_dst, a_src, V)
    if V.dim() not in (2, 3) or a_dst.dim() not in (1, 2) or a_src.dim() not in (1, 2):
        raise ValueError("a_dst and a_src are (rows,) or (rows, heads), V is (rows, dv) or (rows, heads, dv)")
    V3, ad2, as2 = _with_heads(V, 3), _with_heads(a_dst, 2), _with_heads(a_src, 2)
    M, Kk = A.shape
    H, dv = V3.shape[1], V3.shape[2]
    if ad2.shape[1] != H or as2.shape[1] != H:
        raise ValueError("a_dst, a_src and V differ in their number of heads")
    if ad2.shape[0] != M or as2.shape[0] != Kk or V3.shape[0] != Kk or H == 0 or dv == 0:
        raise ValueError("shape mismatch")
    if dv > 128:
        raise ValueError("gat_attention: dv up to 128")
    slope = _check_slope(negative_slope)
    out = _GatAttentionFunction.apply(A, ad2, as2, V3, slope, bool(bias), bool(fast), *_dropout_args(p, seed, step, A.device))
    return _result_like(out, V)


# --- attention from the caller's scores ----------------------------------------------------------------------------------------------
def entry_rows(A):
    """The row of every stored entry of A, in A's entry order: an (nnz,) int64 tensor on A's device -- with A.col_indices() what a score
    f(x[row], x[col]) for score_attention() is computed from.  No host synchronisation."""
    _check_sparse(A, "entry_rows")
    crow, col = _index_tensors(A)
    return torch.repeat_interleave((crow[1:] - crow[:-1]).long(), output_size=col.numel())   # (int32 indices would give int32 rows)


_SCORE_MODES = {"softmax": api.SCORE_SOFTMAX, "none": api.SCORE_WEIGHT}


class _ScoreAttentionFunction(torch.autograd.Function):
    """score_attention(): one kernel pass forward (sextans_score_attention_device), a row pass and a column pass backward
    (sextans_score_attention_backward_device), all heads at once.  S and dS are the only tensors of size nnz; A's values are not read:
    no value refresh anywhere.  Returns (O, lse); lse (softmax mode; else empty) is not differentiable."""

    @staticmethod
    def forward(ctx, A, S, V, mode, fast, p=0.0, seed=0, step=None):
        M, Kk = A.shape
        H, dv = V.shape[1], V.shape[2]
        dvp = _pad8(dv)
        soft = mode == api.SCORE_SOFTMAX
        ent, stream, crow, col, val = _pattern_entry_of(A, fast)
        Sr, lds = _scalars_operand(S.detach())
        Vr, ldv = _heads_operand(V.detach(), dvp)
        O, lse = _out_buffers(A.device, M, H, dvp, lse=soft)
        ent.eng.score_attention_device(mode, H, dvp, Sr.data_ptr(), lds, Vr.data_ptr(), ldv, O.data_ptr(), H * dvp,
                                       lse.data_ptr() if soft else None, _drop_struct(p, seed, step), stream)
        ctx.save_for_backward(crow, col, val, S, V, *((O, lse) if soft else ()))
        _keep_pattern(ctx, A, fast)
        ctx.mode, ctx.dvp = mode, dvp
        ctx.drop = (p, seed, step)   # the backward recomputes the forward's mask
        ctx.mark_non_differentiable(lse)
        return _cut(O, dv), lse

    @staticmethod
    @once_differentiable
    def backward(ctx, G, _):
        crow, col, val, S, V = ctx.saved_tensors[:5]
        O, lse = ctx.saved_tensors[5:] if ctx.mode == api.SCORE_SOFTMAX else (None, None)
        M, Kk = ctx.shape
        H, dv = V.shape[1], V.shape[2]
        dvp = ctx.dvp
        ent, stream = _kept_pattern_entry(ctx, crow, col, val)
        Sr, lds = _scalars_operand(S.detach())
        Vr, ldv = _heads_operand(V.detach(), dvp)
        Gr, ldg = _heads_operand(G, dvp)           # (a copy when G has zero strides, e.g. after .sum(), or dv % 8 != 0)
        dS = _f32(G.device, S.shape[0], H) if ctx.needs_input_grad[1] else None
        dV = _f32(G.device, Kk, H, dvp) if ctx.needs_input_grad[2] else None
        ent.eng.score_attention_backward_device(ctx.mode, H, dvp, Sr.data_ptr(), lds, Vr.data_ptr(), ldv, _ptr(O), H * dvp, _ptr(lse),
                                                Gr.data_ptr(), ldg, _ptr(dS), H, _ptr(dV), H * dvp, _drop_struct(*ctx.drop), stream)
        return None, _cut_grad(dS, H, S), _cut_grad(dV, dv, V), None, None, None, None, None


def score_attention(A, S, V, normalize="softmax", dropout=0.0, seed=None, step=None, return_weights=False, fast=False):
    """Attention on A's pattern from scores the CALLER computed, per head (DGL's edge_softmax + u_mul_e_sum, PyG's softmax(alpha, index) +
    propagate): what HGT, AGNN, SuperGAT, distance / RBF scores, a per-head spatial bias or an MLP on edge features are written with.
        normalize="softmax"   O[r, h, :] = sum over row r's stored entries e = (r, c) of softmax_e(S[:, h] over the row) * V[c, h, :]
        normalize="none"      O[r, h, :] = sum_e S[e, h] * V[c, h, :]   (S holds the weights themselves)
    A (M x Kk) gives the pattern only: its values are not read.  S is (nnz,) or (nnz, H), in A's entry order (entry_rows(A) and
    A.col_indices() give every entry's row and column); V is (Kk, dv) or (Kk, H, dv), the result has V's rank.  One forward call and one
    backward call on the pattern's cached engine for all heads (sextans_score_attention_device / _backward_device), no value refresh,
    nothing of size nnz besides S and its gradient.  Differentiable in S and V; gradients come in the operands' dtypes.  A -inf score
    masks its entry (softmax).  dropout (softmax only), seed and step as in gat_attention_dropout(): made inside the kernels on the
    normalised coefficients; dropout=0 is the plain call, bit for bit.  With normalize="none" the caller holds the weights and drops them.
    return_weights=True (softmax only): also returns the detached (nnz, H) coefficients exp(S - lse[row]) before dropout -- ((nnz,) for
    a 1-D S) -- an elementwise expression on the kernel's log-sum-exp, no kernel of its own.  dv up to 128; a dv that is not a multiple
    of 8, and operands that do not lie as the kernels read them, are copied (V with zero padding)."""
    _check_sparse(A, "score_attention")
    if normalize not in _SCORE_MODES:
        raise ValueError("normalize is 'softmax' or 'none'")
    mode = _SCORE_MODES[normalize]
    _check_dense("score_attention", "S and V", S, V)
    if V.dim() not in (2, 3) or S.dim() not in (1, 2):
        raise ValueError("S is (nnz,) or (nnz, heads), V is (rows, dv) or (rows, heads, dv)")
    V3, S2 = _with_heads(V, 3), _with_heads(S, 2)
    M, Kk = A.shape
    H, dv = V3.shape[1], V3.shape[2]
    if S2.shape[1] != H:
        raise ValueError("S and V differ in their number of heads")
    if S2.shape[0] != A.values().numel() or V3.shape[0] != Kk or H == 0 or dv == 0:
        raise ValueError("shape mismatch")
    if dv > 128:
        raise ValueError("score_attention: dv up to 128")
    p = _check_dropout(dropout)
    if mode != api.SCORE_SOFTMAX and (p > 0.0 or return_weights):
        raise ValueError("normalize='none': the caller holds the weights (no dropout, no return_weights)")
    out, lse = _ScoreAttentionFunction.apply(A, S2, V3, mode, bool(fast), *_dropout_args(p, seed, step, A.device))
    out = _result_like(out, V)
    if not return_weights:
        return out
    w = torch.exp(S2.detach().to(torch.float32) - lse[entry_rows(A)])
    return out, (w if S.dim() == 2 else w[:, 0])


# --- GATv2 ---------------------------------------------------------------------------------------------------------------------------
class _Gatv2AttentionFunction(torch.autograd.Function):
    """gatv2_attention(): one kernel pass forward (sextans_gatv2_attention_device), a row pass, a column pass and the two-level datt sum
    backward (sextans_gatv2_attention_backward_device), all heads at once.  Nothing of size nnz is kept: the backward recomputes the
    scores and the probabilities from the rows' log-sum-exp.  A's values enter as an explicit bias pointer: no value refresh anywhere.
    x_dst and x_src may be the same tensor: autograd adds the two gradients."""

    @staticmethod
    def forward(ctx, A, xdst, xsrc, att, slope, bias, fast, p=0.0, seed=0, step=None):
        M, Kk = A.shape
        H, d = xdst.shape[1], xdst.shape[2]
        dp = _pad8(d)
        ent, stream, crow, col, val = _pattern_entry_of(A, fast)
        xd, ldxd = _heads_operand(xdst.detach(), dp)
        xs, ldxs = _heads_operand(xsrc.detach(), dp)
        at, _ = _heads_operand(att.detach().unsqueeze(0), dp)      # (1, H, dp): heads * dp floats, contiguous
        b, _ = _bias_operands(val, bias)
        O, lse = _out_buffers(A.device, M, H, dp)
        ent.eng.gatv2_attention_dropout_device(H, dp, slope, xd.data_ptr(), ldxd, xs.data_ptr(), ldxs, at.data_ptr(), _ptr(b), O.data_ptr(),
                                               H * dp, lse.data_ptr(), _drop_struct(p, seed, step), stream)
        ctx.save_for_backward(crow, col, val, xdst, xsrc, att, O, lse)
        _keep_pattern(ctx, A, fast)
        ctx.slope, ctx.bias = slope, bias
        ctx.drop = (p, seed, step)   # the backward recomputes the forward's mask
        return _cut(O, d)

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        crow, col, val, xdst, xsrc, att, O, lse = ctx.saved_tensors
        M, Kk = ctx.shape
        H, d = xdst.shape[1], xdst.shape[2]
        dp = O.shape[2]
        ent, stream = _kept_pattern_entry(ctx, crow, col, val)
        xd, ldxd = _heads_operand(xdst.detach(), dp)
        xs, ldxs = _heads_operand(xsrc.detach(), dp)
        at, _ = _heads_operand(att.detach().unsqueeze(0), dp)
        Gr, ldg = _heads_operand(G, dp)           # (a copy when G has zero strides, e.g. after .sum(), or d % 8 != 0)
        b, db = _bias_operands(val, ctx.bias, ctx.needs_input_grad[0])
        new = functools.partial(_f32, G.device)
        delta, dxd, dxs, dat = new(M, H), new(M, H, dp), new(Kk, H, dp), new(H, dp)
        work = new(max(ent.eng.gatv2_workspace_floats(H, dp), 1))
        ent.eng.gatv2_attention_dropout_backward_device(H, dp, ctx.slope, xd.data_ptr(), ldxd, xs.data_ptr(), ldxs, at.data_ptr(), _ptr(b),
                                                        O.data_ptr(), H * dp, lse.data_ptr(), Gr.data_ptr(), ldg, delta.data_ptr(),
                                                        dxd.data_ptr(), H * dp, dxs.data_ptr(), H * dp, dat.data_ptr(), work.data_ptr(),
                                                        _ptr(db), _drop_struct(*ctx.drop), stream)
        need = ctx.needs_input_grad
        return (_pattern_grad(crow, col, val, db, ctx.shape), _cut_grad(dxd, d, xdst, need[1]), _cut_grad(dxs, d, xsrc, need[2]),
                _cut_grad(dat, d, att, need[3]), None, None, None, None, None, None)


def gatv2_attention(A, x_dst, x_src, att, negative_slope=0.2, bias=False, fast=False):
    """GATv2 graph attention (as GATv2Conv in PyG / DGL) on A's pattern, per head:
        softmax over row r's stored entries (r, c) of <att, leaky_relu(x_dst[r] + x_src[c], negative_slope)> [+ A_e], times x_src.
    A (M x Kk) gives the edges -- entry (r, c): source c, destination r -- and, with bias=True, an additive edge term / mask through its
    values, shared by all heads and added after the dot product (-inf masks an edge).  x_dst is (M, H, d), x_src (Kk, H, d), att (H, d);
    or, for one head, (M, d), (Kk, d) and (d,).  The result has x_dst's rank.  The message is x_src itself, as in GATv2Conv; on a square
    pattern x_dst and x_src may be the same tensor (share_weights=True), whose gradient is then the sum of both.
    One kernel pass per direction for all heads (sextans_gatv2_attention_device / sextans_gatv2_attention_backward_device): online
    softmax, nothing of size nnz written -- no (nnz, H, d) tensor of summed rows --, no value refresh; the backward keeps O and M * H
    floats and takes M * H * d floats of workspace for att's gradient, which is summed in a fixed order: the same bits on every run.
    Differentiable in x_dst, x_src, att and (bias=True) A; gradients come in the operands' dtypes.  d up to 128; a d that is not a
    multiple of 8, and operands that do not lie as the kernels read them, are copied with zero padding.  negative_slope: finite, >= 0."""
    return _gatv2_attention(A, x_dst, x_src, att, negative_slope, bias, fast, 0.0, 0, None)


def gatv2_attention_dropout(A, x_dst, x_src, att, dropout, seed=None, step=None, negative_slope=0.2, bias=False, fast=False):
    """gatv2_attention() with dropout on the normalised attention coefficients, as GATv2Conv(dropout=...) in PyG: made inside the fused
    kernels of all three passes (sextans_gatv2_attention_dropout_device / sextans_gatv2_attention_dropout_backward_device).  dropout,
    seed and step as in sparse_attention_dropout(); dropout=0 is gatv2_attention() itself, bit for bit."""
    return _gatv2_attention(A, x_dst, x_src, att, negative_slope, bias, fast, _check_dropout(dropout), seed, step)


def _gatv2_attention(A, x_dst, x_src, att, negative_slope, bias, fast, p, seed, step):
    _check_sparse(A, "gatv2_attention")
    _check_dense("gatv2_attention", "x_dst, x_src and att", x_dst, x_src, att)
    if x_dst.dim() not in (2, 3) or x_src.dim() != x_dst.dim() or att.dim() != x_dst.dim() - 1:
        raise ValueError("x_dst, x_src and att are (rows, heads, d), (rows, heads, d) and (heads, d), or (rows, d), (rows, d) and (d,)")
    xd3, xs3, at2 = _with_heads(x_dst, 3), _with_heads(x_src, 3), (att if att.dim() == 2 else att.unsqueeze(0))
    M, Kk = A.shape
    H, d = xd3.shape[1], xd3.shape[2]
    if xs3.shape[1] != H or at2.shape[0] != H:
        raise ValueError("x_dst, x_src and att differ in their number of heads")
    if xd3.shape[0] != M or xs3.shape[0] != Kk or xs3.shape[2] != d or at2.shape[1] != d or H == 0 or d == 0:
        raise ValueError("shape mismatch")
    if d > 128:
        raise ValueError("gatv2_attention: d up to 128")
    slope = _check_slope(negative_slope)
    out = _Gatv2AttentionFunction.apply(A, xd3, xs3, at2, slope, bool(bias), bool(fast), *_dropout_args(p, seed, step, A.device))
    return _result_like(out, x_dst)
