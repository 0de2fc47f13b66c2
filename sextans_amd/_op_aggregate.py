"""The aggregation ops of the torch front end (private; sextans_amd.torch_op is the public import point): max / min / mean reduce,
softmax aggregation, multi-aggregation, edge-feature SpMM with its multi-aggregation and extrema, and from_edge_index.

All are tiled over N padded up to a multiple of 8; the frame they share -- the way to the cached entry, an optional row-major operand
with its leading dimension, the "is there an element to write" guard, the cut back to N -- is written once in the helpers below."""
import math

import torch
from torch.autograd.function import once_differentiable

from . import api
from ._op_cache import (_check_sparse, _cut, _cut_grad, _f32, _index_tensors, _keep_pattern, _kept_pattern_entry, _pattern_entry_of,
                        _pattern_grad, _ptr, _ptr_nonempty, _qualifies, _row_degrees, _rowmajor, _vals32)
from ._op_product import spmm


# --- the frame of the tiled families -------------------------------------------------------------------------------------------------
def _tiled_entry(A, N, fast):
    """-> (M, K, N padded up to a multiple of 8, the pattern's cached entry, the current stream, A's values)"""
    M, K = A.shape
    ent, stream, _, _, val = _pattern_entry_of(A, fast)
    return M, K, api.round_up_n(N), ent, stream, val


def _rowmajor_ld(t, rows, N, Np, dtype=torch.float32):
    """an optional (rows, N) operand as the kernels read it, zero-padded to Np columns where it must be copied -> (tensor, its leading
    dimension); None -> (None, Np).  dtype: the element type the kernel reads (bf16: an edge tensor of the bf16 entry points)."""
    if t is None:
        return None, Np
    t = _rowmajor(t.detach(), rows, N, Np, dtype)
    return t, t.stride(0)


def _edge_bf16(E, N):
    """does the edge tensor E (nnz, N) go to the bf16 entry points as it lies: bf16, N % 8 == 0, row-major, aligned"""
    return E is not None and E.dtype == torch.bfloat16 and _qualifies(E, N, api.round_up_n(N), torch.bfloat16)


def _any_elements(*outputs):
    """is there any element for a kernel to write (else: no call)"""
    return any(t is not None and t.numel() for t in outputs)


def _check_B(A, B, name):
    if not (isinstance(B, torch.Tensor) and B.is_cuda):
        raise TypeError(name + " expects a CUDA/HIP dense B")
    if B.dim() != 2 or B.shape[0] != A.shape[1] or B.shape[1] == 0:
        raise ValueError("shape mismatch")


# --- max / min / mean ----------------------------------------------------------------------------------------------------------------
_REDUCE_OPS = {"amax": api.REDUCE_MAX, "amin": api.REDUCE_MIN}


def _reduce_forward(A, B, op, fast, want_arg):
    """(C, arg) of the engine's max / min aggregation, both (M, Np) with N padded up to a multiple of 8 (zero columns of B); arg is None
    unless asked for."""
    N = B.shape[1]
    M, K, Np, ent, stream, val = _tiled_entry(A, N, fast)
    Brm, ldb = _rowmajor_ld(B, K, N, Np)
    v = _vals32(val)
    C = _f32(A.device, M, Np)
    arg = torch.empty((M, Np), dtype=torch.int32, device=A.device) if want_arg else None
    ent.eng.spmm_reduce_device_rm(op, Np, _ptr_nonempty(v), _ptr_nonempty(Brm), ldb, _ptr_nonempty(C), Np, _ptr_nonempty(arg), Np, stream)
    return C, arg


class _SpmmReduceFunction(torch.autograd.Function):
    """spmm_reduce(): one kernel pass forward (sextans_spmm_reduce_device_rm) that also records the winning entry of every (row, column),
    a column pass over A^T and a row pass backward (sextans_spmm_reduce_backward_device_rm): every position's gradient goes to the
    entry that won it -- val_e * G to dB, G * B to dA.  A's values enter as an explicit pointer, never through the engine: no value
    refresh anywhere.  Not twice differentiable."""

    @staticmethod
    def forward(ctx, A, B, op, fast):
        N = B.shape[1]
        C, arg = _reduce_forward(A, B, op, fast, True)
        ctx.save_for_backward(*_index_tensors(A), A.values(), B, arg)
        _keep_pattern(ctx, A, fast)
        out_arg = _cut(arg, N)
        ctx.mark_non_differentiable(out_arg)
        return _cut(C, N), out_arg

    @staticmethod
    @once_differentiable
    def backward(ctx, G, _):
        crow, col, val, B, arg = ctx.saved_tensors
        M, K = ctx.shape
        N, Np = B.shape[1], arg.shape[1]
        want_a, want_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_a or want_b):
            return None, None, None, None
        ent, stream = _kept_pattern_entry(ctx, crow, col, val)
        Grm, ldg = _rowmajor_ld(G, M, N, Np)               # (a copy when G has zero strides, e.g. after .sum(), or N % 8 != 0)
        Brm, ldb = _rowmajor_ld(B if want_a else None, K, N, Np)
        v = _vals32(val)
        dB = _f32(G.device, K, Np) if want_b else None
        dv = _f32(G.device, val.numel()) if want_a else None
        if _any_elements(dB, dv):
            ent.eng.spmm_reduce_backward_device_rm(Np, _ptr_nonempty(v), _ptr_nonempty(Brm), ldb, _ptr_nonempty(arg), Np, _ptr_nonempty(Grm),
                                                   ldg, _ptr_nonempty(dB), Np, _ptr_nonempty(dv), stream)
        return _pattern_grad(crow, col, val, dv, ctx.shape), _cut_grad(dB, N, B), None, None


def spmm_reduce(A, B, reduce="amax", return_arg=False, fast=False):
    """The product A B with the sum over a row's entries replaced by another reduction (torch.sparse.mm(A, B, reduce) on the CPU):
    A is an (M, K) sparse_csr matrix, B a dense (K, N) tensor, the result a dense fp32 (M, N) tensor.
    reduce="amax" / "amin": C[r, n] = max / min over row r's stored entries e = (r, c) of A_e * B[c, n] (one rounded fp32 product); a row
    without entries gives 0; stored zeros take part; a NaN product wins.  One kernel pass (sextans_spmm_reduce_device_rm) -- nothing of
    size nnz x N is materialised -- with bits that do not depend on the launch shape or on `fast`, which only selects the cached engine.
    Differentiable in B and in A (dA: a sparse_csr tensor on A's index tensors, in A's value dtype): each position's gradient goes to
    the one entry that won it, the first of equal products, as torch's CPU kernel does.  return_arg=True: also the int32 (M, N) tensor of
    the winning entries' positions in A's CSR arrays (-1 in an empty row; not differentiable).  A's values are handed to the kernel as a
    pointer: no value refresh of the cached engine.  An N that is not a multiple of 8, and a B the kernel cannot read where it lies, are
    copied with zero padding, as spmm() does.
    reduce="mean": spmm(A, B) divided by the rows' entry counts (an empty row: 0); reduce="sum": spmm(A, B).  Both are compositions of
    differentiable ops; return_arg is refused for them."""
    if reduce not in ("amax", "amin", "mean", "sum"):
        raise ValueError("reduce must be 'amax', 'amin', 'mean' or 'sum'")
    if return_arg and reduce in ("mean", "sum"):
        raise ValueError("return_arg needs reduce='amax' or 'amin'")
    if reduce == "sum":
        return spmm(A, B, fast=fast)
    if reduce == "mean":
        out = spmm(A, B, fast=fast)
        return out / _row_degrees(A, out.dtype)
    _check_sparse(A, "spmm_reduce")
    _check_B(A, B, "spmm_reduce")
    op = _REDUCE_OPS[reduce]
    if torch.is_grad_enabled() and (A.requires_grad or B.requires_grad):
        C, arg = _SpmmReduceFunction.apply(A, B, op, bool(fast))
    else:
        C, arg = (_cut(t, B.shape[1]) for t in _reduce_forward(A, B, op, bool(fast), bool(return_arg)))
    return (C, arg) if return_arg else C


# --- softmax aggregation -------------------------------------------------------------------------------------------------------------
def _softagg_forward(A, B, t, fast, want_lse):
    """(C, lse, tp) of the engine's softmax aggregation: C and lse (M, Np) with N padded up to a multiple of 8 (zero columns of B), lse
    None unless asked for; tp the (Np,) fp32 temperatures handed to the kernel (padded columns: 1), None for t = 1 everywhere."""
    N = B.shape[1]
    M, K, Np, ent, stream, val = _tiled_entry(A, N, fast)
    Brm, ldb = _rowmajor_ld(B, K, N, Np)
    v = _vals32(val)
    tp = None
    if t is not None:
        tp = torch.ones((Np,), dtype=torch.float32, device=A.device)
        tp[:N] = t.detach()
    C = _f32(A.device, M, Np)
    lse = _f32(A.device, M, Np) if want_lse else None
    ent.eng.spmm_softagg_device_rm(Np, _ptr_nonempty(v), _ptr_nonempty(Brm), ldb, _ptr(tp), _ptr_nonempty(C), Np, _ptr_nonempty(lse), Np, stream)
    return C, lse, tp


class _SpmmSoftaggFunction(torch.autograd.Function):
    """spmm_softagg(): ONE forward call (sextans_spmm_softagg_device_rm) that keeps C and the log-sum-exp of every (row, column), ONE
    backward call (sextans_spmm_softagg_backward_device_rm) for the gradients that are wanted: a column pass over A^T for dB, a row pass
    for dA and the rows' share of dt, the fixed-order sum over the rows for dt.  t is the (N,) tensor or None (= 1, no gradient); the
    workspace exists only when t wants a gradient.  A's values enter as an explicit pointer: no value refresh.  Not twice differentiable."""

    @staticmethod
    def forward(ctx, A, B, t, fast):
        N = B.shape[1]
        C, lse, tp = _softagg_forward(A, B, t, fast, True)
        ctx.save_for_backward(*_index_tensors(A), A.values(), B, C, lse, *((tp,) if tp is not None else ()))
        _keep_pattern(ctx, A, fast)
        ctx.t_dtype = t.dtype if t is not None else None
        out_lse = _cut(lse, N)
        ctx.mark_non_differentiable(out_lse)
        return _cut(C, N), out_lse

    @staticmethod
    @once_differentiable
    def backward(ctx, G, _):
        crow, col, val, B, C, lse = ctx.saved_tensors[:6]
        tp = ctx.saved_tensors[6] if len(ctx.saved_tensors) > 6 else None
        M, K = ctx.shape
        N, Np = B.shape[1], C.shape[1]
        want_a, want_b, want_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1], tp is not None and ctx.needs_input_grad[2]
        if not (want_a or want_b or want_t):
            return None, None, None, None
        ent, stream = _kept_pattern_entry(ctx, crow, col, val)
        Grm, ldg = _rowmajor_ld(G, M, N, Np)               # (a copy when G has zero strides, e.g. after .sum(), or N % 8 != 0)
        Brm, ldb = _rowmajor_ld(B, K, N, Np)
        v = _vals32(val)
        dB = _f32(G.device, K, Np) if want_b else None
        dv = _f32(G.device, val.numel()) if want_a else None
        dt = _f32(G.device, Np) if want_t else None
        work = _f32(G.device, max(ent.eng.spmm_softagg_workspace_floats(Np), 1)) if want_t else None
        if _any_elements(dB, dv, dt):
            ent.eng.spmm_softagg_backward_device_rm(Np, _ptr_nonempty(v), _ptr_nonempty(Brm), ldb, _ptr_nonempty(tp), _ptr_nonempty(C), Np,
                                                    _ptr_nonempty(lse), Np, _ptr_nonempty(Grm), ldg, _ptr_nonempty(dB), Np, _ptr_nonempty(dv),
                                                    _ptr_nonempty(dt), _ptr_nonempty(work), stream)
        gt = _cut(dt, N).to(ctx.t_dtype) if want_t else None
        return _pattern_grad(crow, col, val, dv, ctx.shape), _cut_grad(dB, N, B), gt, None


def spmm_softagg(A, B, t=1.0, return_lse=False, fast=False):
    """Softmax aggregation (SoftmaxAggregation(t, learn=True) in PyG, the aggregator of GENConv / DeeperGCN): A is an (M, K) sparse_csr
    matrix, B a dense (K, N) tensor, the result a dense fp32 (M, N) tensor
        C[r, n] = sum over row r's stored entries e = (r, c) of softmax_e(t[n] * p_e[n]) * p_e[n],    p_e[n] = A_e * B[c, n]
    -- a softmax per output column over the row's messages themselves (one rounded fp32 product each).  t is the temperature: a Python
    float, a 0-d tensor or an (N,) tensor, any finite values; 0 gives the mean, large values the max, negative ones a soft minimum.  A row
    without entries gives 0.  One kernel pass per direction (sextans_spmm_softagg_device_rm / _backward_device_rm): online softmax, nothing
    of size nnz x N materialised, no atomics -- the same bits on every run.  Differentiable in B, in A (dA: a sparse_csr tensor on A's
    index tensors, in A's value dtype) and in t when it is a tensor that requires grad (a 0-d t gets the sum over the columns); the
    gradients lose digits where |t (p - C)| is large.  return_lse=True: also the (M, N) log-sum-exp of the scores t p (-inf in an empty
    row; not differentiable).  A's values are handed to the kernel as a pointer: no value refresh of the cached engine.  An N that is not
    a multiple of 8, and a B the kernel cannot read where it lies, are copied with zero padding, as spmm_reduce() does; `fast` only selects
    the cached engine."""
    _check_sparse(A, "spmm_softagg")
    _check_B(A, B, "spmm_softagg")
    N = B.shape[1]
    if isinstance(t, torch.Tensor):
        if t.dim() > 1 or (t.dim() == 1 and t.shape[0] != N):
            raise ValueError("t must be a float, a 0-d tensor or an (N,) tensor")
        if not t.is_floating_point():
            raise TypeError("t must be a floating-point tensor")
        tv = t.to(B.device).expand(N)   # (autograd sums a scalar's gradient back)
    elif float(t) == 1.0:
        tv = None                       # the kernels' t == NULL path
    else:
        tv = torch.full((N,), float(t), dtype=torch.float32, device=B.device)
    if torch.is_grad_enabled() and (A.requires_grad or B.requires_grad or (tv is not None and tv.requires_grad)):
        C, lse = _SpmmSoftaggFunction.apply(A, B, tv, bool(fast))
    else:
        C, lse = (_cut(x, N) for x in _softagg_forward(A, B, tv, bool(fast), bool(return_lse))[:2])
    return (C, lse) if return_lse else C


# --- multi-aggregation, of A_e * B[c] or of edge-feature messages -------------------------------------------------------------------
_MULTI_RAW = ("sum", "sumsq", "max", "min")                       # what the kernel computes, in the order of sextans_multi_out
_MULTI_NEEDS = {"sum": ("sum",), "mean": ("sum",), "max": ("max",), "min": ("min",), "sumsq": ("sumsq",),
                "var": ("sum", "sumsq"), "std": ("sum", "sumsq")}   # aggregate -> the raw aggregates it is made of
_EDGE_OPS = {"mul": api.EDGE_MUL, "add": api.EDGE_ADD, "add_relu": api.EDGE_ADD_RELU, "copy": api.EDGE_COPY}


def _multi_raw(A, B, want, place, width, fast, want_arg, E=None, op=None):
    """One forward call of the engine's multi-aggregation.  want: the raw aggregates to compute; place: raw name -> the index of its
    N-column block in an (M, width) output that the kernel writes in place (N % 8 == 0 only; empty: no such output).
    -> (out or None, {raw name not placed: (M, Np) tensor}, argmax, argmin), Np = N padded up to a multiple of 8.
    E (nnz, N) and op (EDGE_*): the edge-feature messages of spmm_edge_multi() instead of A_e * B[c] (B is None for EDGE_COPY)."""
    N = (B if E is None else E).shape[1]
    M, K, Np, ent, stream, val = _tiled_entry(A, N, fast)
    Brm, ldb = _rowmajor_ld(B, K, N, Np)
    v = _vals32(val) if E is None else None
    out = _f32(A.device, M, width) if place else None
    tmp = {name: _f32(A.device, M, Np) for name in want if name not in place}
    args = [torch.empty((M, Np), dtype=torch.int32, device=A.device) if want_arg and name in want else None for name in ("max", "min")]
    if M:
        o = api.MultiOut()
        for name in want:
            if name in place:
                ptr, ld = out.data_ptr() + 4 * N * place[name], width
            else:
                ptr, ld = tmp[name].data_ptr(), Np
            setattr(o, "d_" + name, ptr)
            setattr(o, "ld_" + name, ld)
        o.d_argmax, o.d_argmin = (_ptr(t) for t in args)
        o.ld_arg = Np
        if E is None:
            ent.eng.spmm_multi_device_rm(Np, _ptr_nonempty(v), _ptr_nonempty(Brm), ldb, o, stream)
        else:
            Erm, lde = _rowmajor_ld(E, E.shape[0], N, Np)
            ent.eng.spmm_edge_multi_device_rm(op, Np, _ptr_nonempty(Brm), ldb, _ptr_nonempty(Erm), lde, o, stream)
    return out, tmp, args[0], args[1]


def _multi_grads(ctx, g_out, g_raw, args, M, N, Np):
    """The MultiGrad of a backward call from the upstream gradients that exist: g_out, the gradient of the (M, width) output whose blocks
    ctx.place names, and g_raw, those of the raw aggregates that are tensors of their own; args: the saved args of the extrema in
    ctx.want.  -> (g, the tensors the kernel reads -- to be kept alive over the call --, whether any gradient is given)."""
    arg = dict(zip([name for name in ("max", "min") if name in ctx.want], args))
    g = api.MultiGrad()
    keep = []
    if g_out is not None and ctx.place:
        g_out = _rowmajor(g_out, M, g_out.shape[1], g_out.shape[1])   # (N % 8 == 0 here: the slices are aligned)
        keep.append(g_out)
    for name, gr in zip(_MULTI_RAW, g_raw[:4]):
        if name in ctx.place:
            if g_out is None:
                continue
            ptr, ld = g_out.data_ptr() + 4 * N * ctx.place[name], g_out.stride(0)
        elif gr is not None:
            gr = _rowmajor(gr, M, N, Np)        # (a copy when the gradient has zero strides, e.g. after .sum(), or N % 8 != 0)
            keep.append(gr)
            ptr, ld = gr.data_ptr(), gr.stride(0)
        else:
            continue
        setattr(g, "d_g" + name, ptr)
        setattr(g, "ld_g" + name, ld)
        if name in arg:
            setattr(g, "d_arg" + name, arg[name].data_ptr())
            g.ld_arg = Np
    return g, keep, any(getattr(g, "d_g" + name) for name in _MULTI_RAW)


class _SpmmMultiFunction(torch.autograd.Function):
    """spmm_multi() (E and op None) and spmm_edge_multi() / spmm_edge_reduce(): ONE forward call (sextans_spmm_multi_device_rm /
    sextans_spmm_edge_multi_device_rm) for the raw aggregates that are needed and the args of the extrema, ONE backward call
    (sextans_spmm_multi_backward_device_rm / sextans_spmm_edge_multi_backward_device_rm) that takes the upstream gradients that exist --
    a column pass over A^T for dB and a row pass over A for dA or, with edge features, one that stores dE, each only when autograd asks
    for it.  Without E, A's values enter as an explicit pointer, never through the engine; with E they never enter and A gets no
    gradient: no value refresh anywhere.  Outputs: the (M, width) tensor with the raw aggregates written in place (or None), then sum,
    sumsq, max, min as tensors of their own where they are not placed (else None), argmax, argmin.  Not twice differentiable."""

    @staticmethod
    def forward(ctx, A, B, E, op, want, place, width, fast):
        N = (B if E is None else E).shape[1]
        out, tmp, amax, amin = _multi_raw(A, B, want, place, width, fast, True, E, op)
        ctx.save_for_backward(*_index_tensors(A), A.values(), B, E, *(t for t in (amax, amin) if t is not None))
        _keep_pattern(ctx, A, fast)
        ctx.op, ctx.want, ctx.place = op, want, place
        ctx.set_materialize_grads(False)
        amax, amin = _cut(amax, N), _cut(amin, N)
        ctx.mark_non_differentiable(*(t for t in (amax, amin) if t is not None))
        return (out,) + tuple(_cut(tmp.get(name), N) for name in _MULTI_RAW) + (amax, amin)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, *g_raw):
        crow, col, val, B, E, *args = ctx.saved_tensors
        M, K = ctx.shape
        N = (B if E is None else E).shape[1]
        Np = api.round_up_n(N)
        need = ctx.needs_input_grad
        want_a, want_b, want_e = E is None and need[0], B is not None and need[1], E is not None and need[2]
        none = (None,) * 8
        if not (want_a or want_b or want_e):
            return none
        g, keep, given = _multi_grads(ctx, g_out, g_raw, args, M, N, Np)   # (keep: alive over the call)
        new = torch.empty if given else torch.zeros   # (no upstream gradient at all: zeros, no call)
        dB = new((K, Np), dtype=torch.float32, device=val.device) if want_b else None
        dv = new((val.numel(),), dtype=torch.float32, device=val.device) if want_a else None
        dE = new((E.shape[0], Np), dtype=torch.float32, device=val.device) if want_e else None
        if given and M and _any_elements(dB, dv, dE):   # (else: no element to write)
            ent, stream = _kept_pattern_entry(ctx, crow, col, val)
            if E is None:
                Brm, ldb = _rowmajor_ld(B if (want_a or g.d_gsumsq) else None, K, N, Np)
                ent.eng.spmm_multi_backward_device_rm(Np, _ptr_nonempty(_vals32(val)), _ptr_nonempty(Brm), ldb, g, _ptr_nonempty(dB), Np,
                                                      _ptr_nonempty(dv), stream)
            else:
                Brm, ldb = _rowmajor_ld(B, K, N, Np)
                Erm, lde = _rowmajor_ld(E, E.shape[0], N, Np)
                ent.eng.spmm_edge_multi_backward_device_rm(ctx.op, Np, _ptr_nonempty(Brm), ldb, _ptr_nonempty(Erm), lde, g, _ptr_nonempty(dB), Np,
                                                           _ptr_nonempty(dE), Np, stream)
        elif given:
            for t in (dB, dv, dE):
                if t is not None:
                    t.zero_()
        return (_pattern_grad(crow, col, val, dv, ctx.shape), _cut_grad(dB, N, B), _cut_grad(dE, N, E)) + none[3:]


class _MultiAssemble(torch.autograd.Function):
    """The derived aggregates copied into their N-column blocks of spmm_multi()'s result, in place; backward hands the upstream
    gradient on as it is (the raw aggregates' node reads its own blocks of it) and its blocks to the derived ones as views -- what
    out[:, block] = t would do with a copy of the whole gradient per assignment."""

    @staticmethod
    def forward(ctx, out, blocks, *derived):
        N = derived[0].shape[1]
        for j, t in zip(blocks, derived):
            out[:, j * N:(j + 1) * N] = t
        ctx.blocks, ctx.N = blocks, N
        ctx.mark_dirty(out)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        N = ctx.N
        return (g, None) + tuple(g[:, j * N:(j + 1) * N] for j in ctx.blocks)


def _multi_names(aggr):
    aggr = tuple(aggr)
    if not aggr or any(name not in _MULTI_NEEDS for name in aggr) or len(set(aggr)) != len(aggr):
        raise ValueError("aggr: a non-empty sequence of distinct names out of 'sum', 'mean', 'max', 'min', 'var', 'std', 'sumsq'")
    return aggr


def _multi_plan(aggr, N):
    """-> (the raw aggregates aggr needs, raw name -> its block in the result where the kernel writes it in place, the result's width)"""
    want = tuple(name for name in _MULTI_RAW if any(name in _MULTI_NEEDS[x] for x in aggr))
    place = {name: aggr.index(name) for name in want if name in aggr} if N % 8 == 0 else {}
    return want, place, len(aggr) * N


def _multi_call(A, B, E, op, want, place, width, fast, want_arg):
    """-> (out or None, {raw name: (M, N) tensor}, argmax, argmin) of the multi-aggregation (E and op None) or the edge-feature one,
    through autograd when a gradient can be asked for (the args are then always computed)."""
    N = (B if E is None else E).shape[1]
    if torch.is_grad_enabled() and ((E is None and A.requires_grad) or (B is not None and B.requires_grad) or
                                    (E is not None and E.requires_grad)):
        out, *rest = _SpmmMultiFunction.apply(A, B, E, op, want, place, width, bool(fast))
        return out, {name: t for name, t in zip(_MULTI_RAW, rest[:4]) if t is not None}, rest[4], rest[5]
    out, raw, amax, amin = _multi_raw(A, B, want, place, width, bool(fast), want_arg, E, op)
    return out, {name: _cut(t, N) for name, t in raw.items()}, _cut(amax, N), _cut(amin, N)


def _multi_finish(A, aggr, out, raw, place, N, eps):
    """The result of spmm_multi() / spmm_edge_multi() from the kernel's raw aggregates: the derived ones on top, side by side in aggr's order."""
    for name, j in place.items():
        raw[name] = out[:, j * N:(j + 1) * N]
    got = dict(raw)   # every aggregate that is asked for or needed on the way, from the raw ones
    if any(name in aggr for name in ("mean", "var", "std")):
        deg = _row_degrees(A, torch.float32)
        got["mean"] = raw["sum"] / deg
        if "var" in aggr or "std" in aggr:
            got["var"] = raw["sumsq"] / deg - got["mean"] ** 2
        if "std" in aggr:
            got["std"] = torch.sqrt(torch.relu(got["var"]) + eps)
    if out is None:
        return torch.cat([got[name] for name in aggr], dim=1)
    blocks = tuple(j for j, name in enumerate(aggr) if name not in place)
    return _MultiAssemble.apply(out, blocks, *(got[aggr[j]] for j in blocks)) if blocks else out


def spmm_multi(A, B, aggr=("mean", "max", "min", "std"), eps=1e-5, fast=False):
    """Several aggregations of the same messages at once (PNAConv's aggregators, PyG's MultiAggregation, mean || max read-outs): A is an
    (M, K) sparse_csr matrix, B a dense (K, N) tensor, the result a dense fp32 (M, len(aggr) * N) tensor with the aggregates side by side
    in aggr's order.  The message of the stored entry e = (r, c) is p_e = A_e * B[c, :] (one rounded fp32 product, as in spmm_reduce()).
      "sum", "sumsq", "max", "min": the kernel's own outputs -- sum_e p_e, sum_e p_e^2, and the extrema with the bits of spmm_reduce();
      "mean" = sum / deg, "var" = sumsq / deg - mean^2, "std" = sqrt(relu(var) + eps) (PNA's form), deg the row's stored-entry count
      clamped to at least 1: plain torch elementwise ops on top, differentiated by autograd.  A row without entries gives 0 (std: sqrt(eps)).
    ONE kernel pass gathers B's rows once for everything (sextans_spmm_multi_device_rm), one backward call serves all upstream gradients
    (sextans_spmm_multi_backward_device_rm); differentiable in B and in A (dA: a sparse_csr tensor on A's index tensors); ties send the
    extrema's gradient to the first entry, as spmm_reduce() does.  With N % 8 == 0 the kernel writes "sum", "sumsq", "max" and "min"
    straight into their columns of the result; otherwise operands and results are copied with zero padding, as spmm_reduce() does.  A's
    values are handed over as a pointer: no value refresh of the cached engine.  `fast` only selects the cached engine.  Degree scalers
    are left to the caller."""
    aggr = _multi_names(aggr)
    _check_sparse(A, "spmm_multi")
    _check_B(A, B, "spmm_multi")
    N = B.shape[1]
    want, place, width = _multi_plan(aggr, N)
    out, raw, _, _ = _multi_call(A, B, None, None, want, place, width, fast, False)
    return _multi_finish(A, aggr, out, raw, place, N, eps)


# --- edge-feature SpMM ---------------------------------------------------------------------------------------------------------------
def _edge_forward(A, B, E, op, fast):
    """C (M, Np) of the engine's edge-feature SpMM, N padded up to a multiple of 8 (zero columns of B and E); B is None for EDGE_COPY.
    A bf16 E that the kernel can read where it lies goes to the bf16 entry point as it is: the same bits, no fp32 copy of E."""
    nnz, N = E.shape
    M, K, Np, ent, stream, _ = _tiled_entry(A, N, fast)
    bf16 = _edge_bf16(E, N)
    Brm, ldb = _rowmajor_ld(B, K, N, Np)
    Erm, lde = _rowmajor_ld(E, nnz, N, Np, torch.bfloat16 if bf16 else torch.float32)
    C = _f32(A.device, M, Np)
    if _any_elements(C):
        call = ent.eng.spmm_edge_device_rm_bf16 if bf16 else ent.eng.spmm_edge_device_rm
        call(op, Np, _ptr_nonempty(Brm), ldb, _ptr_nonempty(Erm), lde, _ptr_nonempty(C), Np, stream)
    return C


class _SpmmEdgeFunction(torch.autograd.Function):
    """spmm_edge(): one kernel pass forward (sextans_spmm_edge_device_rm); backward a column pass over A^T for dB and a row pass over A
    that stores dE (sextans_spmm_edge_backward_device_rm).  Only the gradients autograd asks for are computed, and only the operands
    their formulas read are handed over.  A's values never enter: no gradient for A, no value refresh.  Not twice differentiable.
    A bf16 E that went to the bf16 forward as it lies goes to sextans_spmm_edge_backward_device_rm_bf16 the same way, and the kernel
    writes dE in bf16: the bits of the fp32 dE rounded to E's dtype, without the fp32 tensors."""

    @staticmethod
    def forward(ctx, A, B, E, op, fast):
        C = _edge_forward(A, B, E, op, fast)
        ctx.save_for_backward(*_index_tensors(A), A.values(), B, E)
        _keep_pattern(ctx, A, fast)
        ctx.op = op
        return _cut(C, E.shape[1])

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        crow, col, val, B, E = ctx.saved_tensors
        M, K = ctx.shape
        op = ctx.op
        nnz, N = E.shape
        Np = api.round_up_n(N)
        want_b, want_e = B is not None and ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if not (want_b or want_e):
            return None, None, None, None, None
        ent, stream = _kept_pattern_entry(ctx, crow, col, val)
        need_b = op == api.EDGE_ADD_RELU or (op == api.EDGE_MUL and want_e)
        need_e = op == api.EDGE_ADD_RELU or (op == api.EDGE_MUL and want_b)
        bf16 = _edge_bf16(E, N)                            # (the forward's route: one dtype for E and dE)
        e_dtype = torch.bfloat16 if bf16 else torch.float32
        Grm, ldg = _rowmajor_ld(G, M, N, Np)               # (a copy when G has zero strides, e.g. after .sum(), or N % 8 != 0)
        Brm, ldb = _rowmajor_ld(B if need_b else None, K, N, Np)
        Erm, lde = _rowmajor_ld(E if need_e else None, nnz, N, Np, e_dtype)
        dB = _f32(G.device, K, Np) if want_b else None
        dE = torch.empty((nnz, Np), dtype=e_dtype, device=G.device) if want_e else None
        if _any_elements(dB, dE):
            call = ent.eng.spmm_edge_backward_device_rm_bf16 if bf16 else ent.eng.spmm_edge_backward_device_rm
            call(op, Np, _ptr_nonempty(Brm), ldb, _ptr_nonempty(Erm), lde, _ptr_nonempty(Grm), ldg, _ptr_nonempty(dB), Np, _ptr_nonempty(dE), Np,
                 stream)
        return None, _cut_grad(dB, N, B), _cut_grad(dE, N, E), None, None


def _check_edge_op(op):
    if op not in _EDGE_OPS:
        raise ValueError("op must be 'mul', 'add', 'add_relu' or 'copy'")


def _check_edge_operands(A, B, E, op, name, trailing=False):
    """The misuse the edge-feature ops refuse.  trailing: spmm_edge() also takes B (K, H, d) and E (nnz, H, d), the others 2-D operands."""
    _check_edge_op(op)
    _check_sparse(A, name)
    if (B is None) != (op == "copy"):
        raise ValueError(name + ": B=None goes with op='copy', and only with it")
    if not (isinstance(E, torch.Tensor) and E.is_cuda and (B is None or (isinstance(B, torch.Tensor) and B.is_cuda))):
        raise TypeError(name + " expects CUDA/HIP dense B and E")
    if E.dim() not in ((2, 3) if trailing else (2,)) or (B is not None and (B.dim() != E.dim() or B.shape[1:] != E.shape[1:])):
        raise ValueError(name + (": B is (K, N) or (K, H, d), E (nnz, N) or (nnz, H, d) with the same trailing shape" if trailing else
                                 ": B is (K, N), E (nnz, N)"))
    if E.shape[0] != A.values().numel() or (B is not None and B.shape[0] != A.shape[1]) or 0 in E.shape[1:]:
        raise ValueError("shape mismatch")


def spmm_edge(A, B, E, op="mul", reduce="sum", fast=False):
    """Message passing with a feature vector per stored entry: C[r, :] = sum over row r's stored entries e = (r, c) of m_e, where
      op="mul"       m_e = B[c, :] * E[e, :]        (continuous-filter convolution: CFConv, diagonal NNConv; u_mul_e_sum)
      op="add"       m_e = B[c, :] + E[e, :]        (u_add_e_sum)
      op="add_relu"  m_e = relu(B[c, :] + E[e, :])  (GINEConv's aggregation)
      op="copy"      m_e = E[e, :], B=None          (scatter of edge features onto their destination nodes; copy_e_sum)
    A is an (M, K) sparse_csr matrix of which only the PATTERN is used (its values are not read, the cached engine is not refreshed and
    A gets no gradient); B is (K, N) or (K, H, d), E is (nnz, N) or (nnz, H, d) IN A'S CSR ENTRY ORDER (from_edge_index() gives the
    permutation for an edge list); the result has B's trailing shape (E's for "copy"), fp32.  One kernel pass
    (sextans_spmm_edge_device_rm): E is the only tensor of size nnz x N, every message is one rounded fp32 operation, the sums have an
    order fixed by the pattern -- no atomics, the same bits on every run; an empty row gives 0.  reduce="mean": the sum divided by the
    row's entry count clamped to >= 1, a composition.  Differentiable in B and E; only the gradients asked for are computed (a column
    pass over A^T for dB, a row pass that writes dE once).  `fast` only selects the cached engine.  An N that is not a multiple of 8, and
    operands the kernel cannot read where they lie, are copied with zero padding, as spmm() does.  A bf16 E (autocast) with N % 8 == 0
    that is row-major and 16-byte aligned is read as it lies and its gradient written in bf16 by the kernel
    (sextans_spmm_edge_device_rm_bf16 / _backward_device_rm_bf16): the bits of the fp32 route, without an fp32 (nnz, N) tensor."""
    _check_edge_op(op)
    if reduce not in ("sum", "mean"):
        raise ValueError("reduce must be 'sum' or 'mean'")
    _check_edge_operands(A, B, E, op, "spmm_edge", trailing=True)
    M, K = A.shape
    tail = tuple(E.shape[1:])
    B2 = B.reshape(K, math.prod(tail)) if B is not None else None
    E2 = E.reshape(E.shape[0], math.prod(tail))
    code = _EDGE_OPS[op]
    if torch.is_grad_enabled() and ((B2 is not None and B2.requires_grad) or E2.requires_grad):
        out = _SpmmEdgeFunction.apply(A, B2, E2, code, bool(fast))
    else:
        out = _cut(_edge_forward(A, B2, E2, code, bool(fast)), E2.shape[1])
    if reduce == "mean":
        out = out / _row_degrees(A, out.dtype)
    return out.reshape((M,) + tail)


def spmm_edge_multi(A, B, E, op="mul", aggr=("mean", "max", "min", "std"), eps=1e-5, fast=False):
    """Several aggregations of EDGE-FEATURE messages at once: spmm_multi()'s aggregates of spmm_edge()'s messages (PNAConv, whose message
    is an MLP of x_i, x_j and e_ij: op="copy"; MultiAggregation over any materialised message; u_mul_e / u_add_e under several
    reducers).  A is an (M, K) sparse_csr matrix of which only the PATTERN is used, B (K, N) -- None with "copy" --, E (nnz, N) in A's
    CSR entry order; the message of the stored entry e = (r, c) is m_e = B[c] * E[e] ("mul"), B[c] + E[e] ("add"), relu(B[c] + E[e])
    ("add_relu") or E[e] ("copy"), one rounded fp32 operation.  The result is a dense fp32 (M, len(aggr) * N) tensor with the
    aggregates side by side in aggr's order; the names, the derived "mean" / "var" / "std" (eps), the in-place placement for N % 8 == 0
    and the zero padding otherwise are spmm_multi()'s.  ONE kernel pass (sextans_spmm_edge_multi_device_rm), one backward call
    (sextans_spmm_edge_multi_backward_device_rm): nothing of size nnz x N exists besides E and its gradient, no atomics, the same bits on
    every run.  Differentiable in B and E; ties send the extrema's gradient to the first entry.  A gets no gradient and the cached
    engine no value refresh.  `fast` only selects the cached engine."""
    aggr = _multi_names(aggr)
    _check_edge_operands(A, B, E, op, "spmm_edge_multi")
    N = E.shape[1]
    want, place, width = _multi_plan(aggr, N)
    out, raw, _, _ = _multi_call(A, B, E, _EDGE_OPS[op], want, place, width, fast, False)
    return _multi_finish(A, aggr, out, raw, place, N, eps)


def spmm_edge_reduce(A, B, E, op="mul", reduce="amax", return_arg=False, fast=False):
    """The max ("amin": the min) over a row's entries of spmm_edge()'s messages: C[r, n] = max over row r's stored entries e = (r, c)
    of m_e[n] (EdgeConv / DGCNN: copy_e_max; DGL's u_mul_e_max, u_add_e_max).  Operands, ops and messages as spmm_edge_multi(), of which
    this is the extrema group with one output: a dense fp32 (M, N) tensor; a row without entries gives 0, a NaN message wins, the first
    of equal messages wins.  return_arg=True: also the int32 (M, N) tensor of the winning entries' positions in A's CSR arrays (= rows
    of E; -1 in an empty row; not differentiable).  Differentiable in B and E: each position's gradient goes to the entry that won it."""
    if reduce not in _REDUCE_OPS:
        raise ValueError("reduce must be 'amax' or 'amin'")
    _check_edge_operands(A, B, E, op, "spmm_edge_reduce")
    name = "max" if reduce == "amax" else "min"
    _, raw, amax, amin = _multi_call(A, B, E, _EDGE_OPS[op], (name,), {}, E.shape[1], fast, bool(return_arg))
    return (raw[name], amax if name == "max" else amin) if return_arg else raw[name]


def from_edge_index(edge_index, num_dst, num_src, values=None):
    """The sparse_csr matrix of an edge list, and the permutation that brings per-edge data into its entry order.
    edge_index: (2, nnz) integers, row 0 the SOURCE and row 1 the DESTINATION of every edge (PyG's convention): edge i is the entry
    A[dst_i, src_i] of the (num_dst, num_src) matrix.  The edges are sorted stably by (dst, src).  Returns (A, perm): A's values are
    values[perm] (ones when values is None), and edge_attr[perm] is the E of spmm_edge() in A's entry order.  A duplicate edge raises
    ValueError (multigraphs: not supported).  Plain torch; run it once per graph."""
    if not isinstance(edge_index, torch.Tensor) or edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.is_floating_point():
        raise ValueError("edge_index must be a (2, nnz) integer tensor")
    num_dst, num_src = int(num_dst), int(num_src)
    nnz = edge_index.shape[1]
    src, dst = edge_index[0].long(), edge_index[1].long()
    if nnz and (int(src.min()) < 0 or int(src.max()) >= num_src or int(dst.min()) < 0 or int(dst.max()) >= num_dst):
        raise ValueError("edge_index out of range")
    if values is not None and values.shape[0] != nnz:
        raise ValueError("values must have one element per edge")
    key, perm = torch.sort(dst * num_src + src, stable=True)
    if nnz > 1 and bool((key[1:] == key[:-1]).any()):
        raise ValueError("from_edge_index: duplicate edge (multigraphs are not supported)")
    itype = torch.int32 if max(num_dst, num_src, nnz) < 2 ** 31 else torch.int64
    crow = torch.zeros(num_dst + 1, dtype=torch.int64, device=edge_index.device)
    crow[1:] = torch.cumsum(torch.bincount(dst, minlength=num_dst), 0)
    vals = values[perm] if values is not None else torch.ones(nnz, dtype=torch.float32, device=edge_index.device)
    A = torch.sparse_csr_tensor(crow.to(itype), src[perm].to(itype), vals, size=(num_dst, num_src))
    return A, perm
