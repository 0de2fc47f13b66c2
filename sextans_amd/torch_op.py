"""Operator-style embedding: torch.sparse_csr in, dense out, over the C ABI.

    C = spmm(A_csr, B, alpha=1.0, beta=0.0, C=None)

A: torch.sparse_csr_tensor (fp32 values, int32/int64 indices) on a GPU; B: dense (K, N) fp32; returns a
dense (M, N) tensor.  Torch tensors are ROW-major, and so is the entry point used here (sextans_spmm_device_rm, round 5): a
contiguous fp32 B with N % 8 == 0 is handed to the kernel where it lies -- for N = 16 it IS the kernel's B panel -- and the
result is written straight into the (M, N) tensor that is returned: no transposes, no copies.  (Until round 4 this op transposed B
into a column-major copy that the engine repacked into row-major panels again, and C likewise in reverse: two passes over B and two
over C per call.)  N that is not a multiple of 8 is padded up internally (the reference's N-tile granularity, sextans-host.cpp:51).  One cached engine per live
sparsity pattern (keyed on the index tensors' addresses, their contents re-checked when their version counters move; the entry pins the tensors, at most 8 kept, clear_cache()
drops them); new VALUES on a cached pattern are a refresh of the engine's copies, not a new engine (refresh(), cache_info()); not part
of the reference, whose only front end is the CLI.

Attention over a fixed sparsity pattern (graph attention, sparse / sliding-window attention) on the same cached engine:

    S = sddmm(A, X, Y, alpha=1.0, beta=0.0)        S_e = alpha * <X[r, :], Y[c, :]> + beta * A_e on A's pattern
    P = row_softmax(S, scale=1.0)                  softmax over every row's stored entries
    O = sparse_attention(A, Q, K, V, scale=None, bias=False)  = spmm(row_softmax(sddmm(A, Q, K, beta=bias), scale), V)
    O = sparse_attention(A, Q, K, V, ..., fused=True)         the same in one kernel pass per direction, all heads of (rows, H, d) at once
    O = gat_attention(A, a_dst, a_src, V, negative_slope=0.2, bias=False)   graph attention (GATConv): the additive score
                                                   softmax(leaky_relu(a_dst[r] + a_src[c] [+ A_e])) V per head, fused the same way
    O = gatv2_attention(A, x_dst, x_src, att, negative_slope=0.2, bias=False)   GATv2 (GATv2Conv): the activation inside the projection
                                                   softmax(<att, leaky_relu(x_dst[r] + x_src[c])> [+ A_e]) x_src per head, fused the same way
    O = score_attention(A, S, V, normalize="softmax", dropout=0.0, seed=None, step=None, return_weights=False)
                                                   any OTHER score: S is (nnz, H), computed by the caller in A's entry order; softmax over
                                                   each row per head, times V (edge_softmax + u_mul_e_sum) -- or normalize="none": S holds
                                                   the weights themselves.  One kernel pass per direction, differentiable in S and V
    rows = entry_rows(A)                           the (nnz,) row of every stored entry: S = f(x[rows], x[A.col_indices()])

Dropout on the normalised attention coefficients (GATConv / GATv2Conv's dropout, attn_drop), made INSIDE the fused kernels from a hash
of (seed, step, entry, head) -- the coefficients are never materialised, so it cannot be applied from outside:

    O = sparse_attention_dropout(A, Q, K, V, dropout, seed=None, step=None, scale=None, bias=False, fast=False, fused=False)
    O = gat_attention_dropout(A, a_dst, a_src, V, dropout, seed=None, step=None, negative_slope=0.2, bias=False, fast=False)
    O = gatv2_attention_dropout(A, x_dst, x_src, att, dropout, seed=None, step=None, negative_slope=0.2, bias=False, fast=False)
    m = dropout_mask(A, heads, p, seed, step=None)   the (nnz, heads) multipliers themselves: 1 / (1 - p) or 0

Max / min / mean aggregation over a node's neighbours (GraphSAGE-pool, PNA, EdgeConv; torch.sparse.mm(A, B, reduce) on the CPU, reduce="max"
in PyG, copy_u_max in DGL), again on the cached engine of the pattern:

    C = spmm_reduce(A, B, reduce="amax")           C[r, n] = max ("amin": min) over row r's stored entries (r, c) of A_e * B[c, n]; an empty
                                                   row gives 0.  One kernel pass, nothing of size nnz x N materialised; return_arg=True
                                                   also returns the winning entries.  "mean" / "sum": spmm() (divided by the row lengths)
    C = spmm_multi(A, B, aggr=("mean", "max", "min", "std"))   several aggregations of the same messages side by side, (M, len(aggr) N)
                                                   (PNAConv, MultiAggregation): one kernel pass gathers B's rows once for the sum, the sum
                                                   of squares, the max and the min; one backward call.  Also "sum", "var", "sumsq"
    C = spmm_softagg(A, B, t=1.0)                  softmax aggregation (SoftmaxAggregation(t, learn=True), GENConv): a softmax per column over
                                                   the row's messages, weighted sum of the same messages; differentiable in A, B and t

Edge-feature message passing -- a feature VECTOR per stored entry instead of a scalar weight (SchNet's CFConv / diagonal NNConv, GINEConv,
the edge -> node reduction of MeshGraphNets; u_mul_e_sum, u_add_e_sum, copy_e_sum in DGL), on the cached engine of the pattern:

    C = spmm_edge(A, B, E, op="mul", reduce="sum") C[r, n] = sum over row r's stored entries e = (r, c) of B[c, n] * E[e, n] ("add": B + E,
                                                   "add_relu": relu(B + E), "copy": E[e, n], B=None); E is (nnz, N) in A's entry order.  One
                                                   kernel pass per direction, E the only nnz x N tensor, no atomics; "mean": / row length
    C = spmm_edge_multi(A, B, E, op="mul", aggr=("mean", "max", "min", "std"))   spmm_multi()'s aggregates of spmm_edge()'s messages,
                                                   (M, len(aggr) N): PNAConv over an edge MLP's messages ("copy"), MultiAggregation; one
                                                   kernel pass, one backward call, nothing of size nnz x N beyond E and dE
    C = spmm_edge_reduce(A, B, E, op="mul", reduce="amax")   the max ("amin": min) of those messages alone (EdgeConv / DGCNN: copy_e_max,
                                                   u_mul_e_max, u_add_e_max); return_arg=True also returns the winning entries
    A, perm = from_edge_index(edge_index, num_dst, num_src)   the sparse_csr A of a PyG edge list, and perm with E = edge_attr[perm]

Edge features INSIDE the fused attention (TransformerConv(edge_dim=...), UniMP, relative-position encodings), one kernel pass per direction:

    O = sparse_attention_edge(A, Q, K, V, edge_key=None, edge_value=None, scale=None, bias=False, dropout=0.0, seed=None, step=None)
                                                   softmax(scale * (<Q[r], K[c] + edge_key[e]> [+ A_e])) (V[c] + edge_value[e]) per head;
                                                   the edge tensors are (nnz, H, d) in A's entry order; edge_key is edge_value: one gradient

S and P are sparse_csr tensors that carry A's own index tensors, so the three ops and spmm() meet in one cache entry and hand each
other's values to the engine as value refreshes; all are differentiable, their backward passes run on the engine too.
"""
import collections
import math
import weakref

import torch
from torch.autograd.function import once_differentiable

from . import api

_MAX_ENGINES = 8
_cache = collections.OrderedDict()     # key -> _Entry
_counters = {"engines_built": 0, "value_refreshes": 0}


class _Entry:
    """An engine, the arrays it reads (it does not copy: they are kept alive here), A's own index tensors (pinned, so their addresses
    cannot be recycled for another pattern while the entry lives), what the index tensors looked like when the engine was built
    (version counters + a fingerprint of their contents) and the value tensor the engine last saw."""
    __slots__ = ("eng", "crow32", "col32", "val32", "crow", "col", "val", "idx_ver", "idx_fp", "val_ptr", "val_ver")

    def __getitem__(self, i):   # tests/test_torch_op_gpu.py reads the engine of an entry as entry[0]: (engine, engine's arrays, A's tensors)
        return (self.eng, (self.crow32, self.col32, self.val32), (self.crow, self.col, self.val))[i]


def _ver(t):   # inference-mode tensors have no version counter
    try:
        return t._version
    except RuntimeError:
        return None


_FP_CHUNK = 1 << 24   # indices per pass of the fingerprint: 64 MiB of int32 temporaries whatever nnz is


def _fingerprint(crow, col):
    """Three 32-bit sums (wrapping) over the index tensors, read back once: tells an in-place change of the PATTERN from an in-place change
    of the values -- the members of one sparse tensor share a single version counter, so A.values().mul_(2) moves the counters of
    A.crow_indices() and A.col_indices() too.  Computed in chunks of _FP_CHUNK indices in int32, so it reads the indices once and
    allocates a few chunk-sized temporaries, not a multiple of nnz; the read-back synchronises (not possible under stream capture)."""
    acc = torch.zeros(3, dtype=torch.int32, device=col.device)
    acc[0] = crow.to(torch.int32).sum(dtype=torch.int32)
    w = torch.arange(1, min(_FP_CHUNK, max(col.numel(), 1)) + 1, device=col.device, dtype=torch.int32) % 65521 + 1
    for i in range(0, col.numel(), _FP_CHUNK):
        c = col[i:i + _FP_CHUNK].to(torch.int32)
        acc[1] += c.sum(dtype=torch.int32)
        acc[2] += (c * w[:c.numel()] + (i // _FP_CHUNK)).sum(dtype=torch.int32)
    return tuple(acc.tolist())


def _evict(key):
    ent = _cache.pop(key, None)
    if ent is not None:
        ent.eng.close()


def clear_cache():
    """Drop every cached engine (and the references that pin the matrices they were built from); resets cache_info()."""
    for key in list(_cache):
        _evict(key)
    _counters["engines_built"] = _counters["value_refreshes"] = 0


def cache_info():
    """Process-wide counters since the last clear_cache(): engines built (pattern analysis + planning), value refreshes served on a cached
    engine instead (Engine.update_values_device), and the entries alive now."""
    return {"engines_built": _counters["engines_built"], "value_refreshes": _counters["value_refreshes"], "entries": len(_cache)}


_carried = {}   # id(T) -> (weak reference to T, A's crow, A's col, T's index version counters): sparse results of the ops below


def _carry(T, crow, col):
    """Remember that the sparse tensor T was built on (crow, col), the index tensors a cache entry remembers.  The index members of a
    newly built sparse tensor have version counters of their own, which say nothing to the cache: it would fall back to the
    fingerprint (a read-back) on every call of a pipeline.  The ops look the remembered tensors up by T's identity instead."""
    key = id(T)
    _carried[key] = (weakref.ref(T, lambda _, key=key: _carried.pop(key, None)), crow, col, (_ver(T.crow_indices()), _ver(T.col_indices())))
    return T


def _index_tensors(A):
    """A's index tensors -- for a result of sddmm() / row_softmax() that nobody has written to since, the ones it was built on."""
    c = _carried.get(id(A))
    if c is not None and c[0]() is A and None not in c[3] and (_ver(A.crow_indices()), _ver(A.col_indices())) == c[3]:
        return c[1], c[2]
    return A.crow_indices(), A.col_indices()


def _engine_for(A, dev, fast=False):
    crow, col = _index_tensors(A)
    return _engine_for_parts(crow, col, A.values(), tuple(A.shape), dev, fast)


def _refresh_entry(ent, val):
    """New values onto the entry's engine, on the current stream: copy kernels over the packed forms that exist, nothing planned again."""
    val32 = val.to(torch.float32).contiguous()   # (val itself when it is fp32 and contiguous: the engine then reads A's own storage)
    ent.eng.update_values_device(val32.data_ptr(), torch.cuda.current_stream(val.device).cuda_stream)
    ent.val32, ent.val, ent.val_ptr, ent.val_ver = val32, val, val.data_ptr(), _ver(val)
    _counters["value_refreshes"] += 1


def _engine_for_parts(crow, col, val, shape, dev, fast=False, force_refresh=False):
    return _entry_for_parts(crow, col, val, shape, dev, fast, force_refresh).eng


def _entry_for_parts(crow, col, val, shape, dev, fast=False, force_refresh=False, values_needed=True):
    """One engine per sparsity PATTERN, at most _MAX_ENGINES of them (LRU: every entry pins an engine with its device workspaces).
    The key holds the addresses of A's INDEX tensors, the shape, nnz, device and mode -- not the values: what is expensive to build
    (block dictionaries, clustering, the sort behind A^T) depends on the pattern alone.  The entry keeps A's index tensors alive: as
    long as it exists their storage cannot be freed and handed to a different pattern, so equal addresses mean the same storage.
      Index tensors whose version counters have not moved since the engine was built hold the same pattern.  Counters that moved (the
    members of one sparse tensor share ONE counter, so an in-place update of A.values() moves them too) or that do not exist (inference
    mode) say nothing: the contents are compared through a fingerprint (one pass over the indices, one read-back -- it synchronises,
    so it cannot happen inside a stream capture, and a training step that updates A.values() in place pays it on its next spmm(), on
    top of the engine's value refresh); a changed pattern gets a new engine, as ever.
      The entry remembers the value tensor it last served (address + version).  A call that finds other values -- an optimizer step in
    place, another value tensor on the same pattern, values without a version counter (every call) -- refreshes the engine's copies on
    the current stream (sextans_update_values_device) instead of building an engine.  What the counters cannot see is a change made
    through ANOTHER alias of the value storage (the dense tensor A was built from): refresh(A) is for that.
      values_needed=False (row_softmax: the pattern alone matters) leaves the values of a cached engine as they are."""
    M, K = shape
    key = (dev, crow.data_ptr(), col.data_ptr(), M, K, val.numel(), bool(fast))
    ivers = (_ver(crow), _ver(col))
    ent = _cache.get(key)
    if ent is not None:
        if None in ivers or ivers != ent.idx_ver:
            if _fingerprint(crow, col) == ent.idx_fp:
                ent.idx_ver = ivers
            else:
                _evict(key)
                ent = None
    if ent is not None:
        _cache.move_to_end(key)
        vv = _ver(val)
        if values_needed and (force_refresh or vv is None or vv != ent.val_ver or val.data_ptr() != ent.val_ptr):
            _refresh_entry(ent, val)
        return ent
    ent = _Entry()
    ent.crow32, ent.col32 = crow.to(torch.int32).contiguous(), col.to(torch.int32).contiguous()
    ent.val32 = val.to(torch.float32).contiguous()
    ent.crow, ent.col, ent.val, ent.val_ptr, ent.val_ver = crow, col, val, val.data_ptr(), _ver(val)
    ent.idx_ver, ent.idx_fp = ivers, _fingerprint(crow, col)
    ent.eng = eng = api.Engine(dev)
    if fast:   # SEXTANS_MODE_FAST: FMA + re-associated hub rows, |d| <= 1e-4 * (|alpha| sum|a b| + |beta c|); the default is bit identity with cpu_spmm_CSR
        eng.set_option("mode", 1)
    eng.set_matrix_csr_device(M, K, ent.val32.numel(), ent.crow32.data_ptr(), ent.col32.data_ptr(), ent.val32.data_ptr())
    _counters["engines_built"] += 1
    _cache[key] = ent
    while len(_cache) > _MAX_ENGINES:
        _evict(next(iter(_cache)))
    return ent


def refresh(A, fast=False):
    """Unconditionally bring the cached engine of A (created if there is none) up to A's current values, on the current stream.  spmm()
    notices values changed through A's own tensors by itself (version counter) -- but inside a captured step no Python runs on replay:
    a capture of refresh(A); out = spmm(A, B); out.backward(G); values -= lr * dA replays as a complete training step, the refresh
    kernels re-reading A's value storage every time.  Also for values changed through another alias of A's value storage, which no
    version counter of A shows.
      Before CAPTURING such a step call refresh(A) once OUTSIDE the capture, after the last in-place update of A.values(): that update
    moved the version counter A's index tensors share with its values, and the check that follows (a fingerprint of the indices, read
    back to the host) synchronises, which a stream capture refuses.  Inside the capture the counters are then as remembered and
    refresh(A) only enqueues the copy kernels."""
    if A.layout != torch.sparse_csr or not A.is_cuda:
        raise TypeError("refresh expects a CUDA/HIP torch.sparse_csr matrix")
    _engine_for_parts(A.crow_indices(), A.col_indices(), A.values(), tuple(A.shape), A.device.index or 0, fast, force_refresh=True)


def _qualifies(t, cols, colsp, dtype):
    """dtype, unit column stride, 16-byte aligned base and row stride (4 fp32 / 8 bf16 elements): the engine reads or writes it where it lies"""
    per16 = 4 if dtype == torch.float32 else 8
    return (t.dtype == dtype and cols == colsp and t.stride(1) == 1 and t.stride(0) >= cols and t.stride(0) % per16 == 0 and
            t.data_ptr() % 16 == 0)


def _rowmajor(t, rows, cols, colsp, dtype=torch.float32):
    """the tensor itself when it qualifies, else a padded copy in `dtype`"""
    if _qualifies(t, cols, colsp, dtype):
        return t
    out = torch.zeros((rows, colsp), dtype=dtype, device=t.device)
    out[:, :cols] = t
    return out


def spmm(A, B, alpha=1.0, beta=0.0, C=None, out=None, fast=False, transpose_a=False, out_dtype=None):
    """out (optional): an (M, N) row-major tensor of the result's dtype that receives the result (N % 8 == 0); may be C itself (in place).
    fast (round 6): the engine's documented in-tolerance mode (include/sextans_amd.h, SEXTANS_MODE_FAST) instead of bit identity with the
    reference's cpu_spmm_CSR; a matrix used in both modes keeps one engine per mode.
    transpose_a: alpha * A^T * B + beta * C with B (M, N) and C (K, N) (sextans_spmm_t_device_rm).
    bf16: a bf16 B that the engine can read where it lies (unit column stride, 16-byte aligned, N % 8 == 0, row stride % 8 == 0) goes to
    the bf16 entry point (sextans_spmm_device_rm_bf16) without an fp32 copy; the result is still fp32 with the bits of spmm(A, B.float()),
    since widening is exact.  out_dtype (None = torch.float32, or torch.bfloat16): with torch.bfloat16 the result (and out=) is bf16: the fp32
    result rounded to nearest even, once, whatever the dtypes and alignment of B and C (a bf16 C is widened exactly and, with a bf16 B, read
    by the engine as it is; an fp32 C is never rounded; with an fp32 B or an fp32 C: the fp32 result and one rounding pass).
    Differentiable: with grad mode on and A (its values), B or C requiring grad the call is an autograd node (_SpmmFunction) whose
    backward runs on the engine -- dB through the transposed (or, for transpose_a, the forward) product, dA through the SDDMM kernel on
    A's pattern, dC = beta * G; out= is refused then, as by torch's own out= ops.  A bf16 upstream gradient feeds the dB product through
    the bf16 entry point, and dB is written in bf16 directly when B is bf16."""
    if A.layout != torch.sparse_csr or not A.is_cuda or not B.is_cuda:
        raise TypeError("spmm expects a CUDA/HIP torch.sparse_csr matrix and a CUDA/HIP dense B")
    if out_dtype not in (None, torch.float32, torch.bfloat16):
        raise TypeError("out_dtype must be None, torch.float32 or torch.bfloat16")
    if torch.is_grad_enabled() and (A.requires_grad or B.requires_grad or (C is not None and C.requires_grad)):
        if out is not None:
            raise RuntimeError("spmm(): functions with out=... arguments don't support automatic differentiation, but one of the "
                               "arguments requires grad")
        return _SpmmFunction.apply(A, B, C, float(alpha), float(beta), bool(fast), bool(transpose_a), out_dtype)
    return _forward(A, B, alpha, beta, C, out, fast, transpose_a, out_dtype)


def _forward(A, B, alpha, beta, C, out, fast, transpose_a, out_dtype=None):
    M, K = A.shape
    rows_b, rows_c = (M, K) if transpose_a else (K, M)
    if B.dim() != 2 or B.shape[0] != rows_b:
        raise ValueError("shape mismatch")
    N = B.shape[1]
    Np = api.round_up_n(N)
    dev = A.device.index or 0
    eng = _engine_for(A, dev, fast)
    odt = torch.float32 if out_dtype is None else out_dtype
    b16 = _qualifies(B, N, Np, torch.bfloat16)          # B as it lies, on the bf16 entry point
    # dtype of the C buffers the engine works on: bf16 only where that rounds nothing but the result -- an fp32 C is never rounded before
    # the product (it stays fp32 on the bf16 entry and the result is rounded once, below), so the bits do not depend on where B lies
    c_given = C is not None and beta != 0.0
    cdt = torch.bfloat16 if b16 and odt == torch.bfloat16 and (not c_given or C.dtype == torch.bfloat16) else torch.float32
    Brm = B if b16 else _rowmajor(B, rows_b, N, Np)
    if c_given:
        if tuple(C.shape) != (rows_c, N):
            raise ValueError("shape mismatch")
        Cin = _rowmajor(C, rows_c, N, Np, cdt)
    else:
        Cin = None
    if out is not None and (tuple(out.shape) != (rows_c, N) or not _qualifies(out, N, Np, odt)):
        raise ValueError("out must be an (M, N) %s row-major tensor with N %% 8 == 0, 16-byte aligned" % ("fp32" if odt == torch.float32 else "bf16"))
    eng_out = out if cdt == odt else None               # (fp32 B or fp32 C with a bf16 out: the engine writes fp32, the rounding pass fills out)
    Cout = eng_out if eng_out is not None else (Cin if (Cin is not None and Cin is not C) else None)
    if Cout is None:       # beta * C_in with C_in = 0 when no C is given: zeros, also for beta == 0 (0 * NaN would not be 0)
        Cout = torch.zeros((rows_c, Np), dtype=cdt, device=B.device) if Cin is None else torch.empty((rows_c, Np), dtype=cdt, device=B.device)
    if Cin is None:
        if eng_out is not None:
            eng_out.zero_()
        Cin = Cout
    stream = torch.cuda.current_stream(B.device).cuda_stream
    if b16:
        call = eng.spmm_t_device_rm_bf16 if transpose_a else eng.spmm_device_rm_bf16
        call(Np, float(alpha), Brm.data_ptr(), Brm.stride(0), float(beta), Cin.data_ptr(), Cin.stride(0), Cout.data_ptr(), Cout.stride(0),
             api.DTYPE_BF16 if cdt == torch.bfloat16 else api.DTYPE_F32, stream)
    else:
        call = eng.spmm_t_device_rm if transpose_a else eng.spmm_device_rm
        call(Np, float(alpha), Brm.data_ptr(), Brm.stride(0), float(beta), Cin.data_ptr(), Cin.stride(0), Cout.data_ptr(), Cout.stride(0), stream)
    res = Cout if Np == N else Cout[:, :N]
    if cdt != odt:
        if out is None:
            return res.to(odt)
        out.copy_(res)
        return out
    return res


class _SpmmFunction(torch.autograd.Function):
    """C_out = alpha * op(A) * B + beta * C with op(A) = A or A^T.  With upstream gradient G:
         dB = alpha * op(A)^T * G         the transposed entry on the cached engine (transpose_a: the forward entry)
         dA = alpha * (G B^T or B G^T)    sampled on A's pattern: the SDDMM kernel, a CSR gradient in A's index and value dtypes
         dC = beta * G
    The backward reads A's index / value tensors and B: saved with save_for_backward, so an in-place change of either between forward
    and backward raises torch's version error.  Not twice differentiable."""

    @staticmethod
    def forward(ctx, A, B, C, alpha, beta, fast, transpose_a, out_dtype=None):
        out = _forward(A, B, alpha, beta, C, None, fast, transpose_a, out_dtype)
        ctx.save_for_backward(*_index_tensors(A), A.values(), B)
        ctx.shape, ctx.alpha, ctx.beta, ctx.fast, ctx.transpose_a = tuple(A.shape), alpha, beta, fast, transpose_a
        ctx.dev = A.device.index or 0
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        crow, col, val, B = ctx.saved_tensors
        M, K = ctx.shape
        N = G.shape[1]
        Np = api.round_up_n(N)
        eng = _engine_for_parts(crow, col, val, ctx.shape, ctx.dev, ctx.fast)
        stream = torch.cuda.current_stream(G.device).cuda_stream
        rows_b, rows_g = (M, K) if ctx.transpose_a else (K, M)
        gA = gB = gC = None
        if ctx.needs_input_grad[1]:
            if _qualifies(G, N, Np, torch.bfloat16):   # bf16 upstream gradient as it lies; dB in bf16 directly when B is bf16
                odt = torch.bfloat16 if B.dtype == torch.bfloat16 else torch.float32
                out = torch.zeros((rows_b, Np), dtype=odt, device=G.device)
                call = eng.spmm_device_rm_bf16 if ctx.transpose_a else eng.spmm_t_device_rm_bf16
                call(Np, ctx.alpha, G.data_ptr(), G.stride(0), 0.0, out.data_ptr(), Np, out.data_ptr(), Np,
                     api.DTYPE_BF16 if odt == torch.bfloat16 else api.DTYPE_F32, stream)
            else:
                Grm = _rowmajor(G, rows_g, N, Np)      # (a copy when G has zero strides, e.g. after .sum(), or N % 8 != 0)
                out = torch.zeros((rows_b, Np), dtype=torch.float32, device=G.device)
                call = eng.spmm_device_rm if ctx.transpose_a else eng.spmm_t_device_rm
                call(Np, ctx.alpha, Grm.data_ptr(), Grm.stride(0), 0.0, out.data_ptr(), Np, out.data_ptr(), Np, stream)
            gB = (out if Np == N else out[:, :N]).to(B.dtype)
        if ctx.needs_input_grad[0]:
            Grm = _rowmajor(G, rows_g, N, Np)          # (the SDDMM kernel reads fp32)
            Brm = _rowmajor(B, rows_b, N, Np)  # (zero padding adds +0 products: +0 + +0 keeps every sum's bits)
            X, Y = (Brm, Grm) if ctx.transpose_a else (Grm, Brm)
            vals = torch.empty((val.numel(),), dtype=torch.float32, device=G.device)
            if vals.numel():
                eng.sddmm_device_rm(Np, ctx.alpha, X.data_ptr(), X.stride(0), Y.data_ptr(), Y.stride(0), 0.0, None, vals.data_ptr(), stream)
            gA = torch.sparse_csr_tensor(crow, col, vals.to(val.dtype), size=(M, K))
        if ctx.needs_input_grad[2]:
            gC = G * ctx.beta if ctx.beta != 0.0 else torch.zeros_like(G)
        return gA, gB, gC, None, None, None, None, None


def _vals32(v):
    """fp32, contiguous, 16-byte aligned: v itself where it is all that"""
    v = v.detach().to(torch.float32).contiguous()
    return v if v.data_ptr() % 16 == 0 else v.clone()


def _grad_values(G, crow, col, nnz):
    """The values of a gradient on A's pattern, in A's entry order: a CSR gradient built on the pattern (what every backward here and
    torch's own sparse ops return), or a dense one, gathered."""
    if G.layout == torch.sparse_csr:
        if G.values().numel() != nnz:
            raise ValueError("gradient on another sparsity pattern")
        return _vals32(G.values())
    rows = torch.repeat_interleave(torch.arange(crow.numel() - 1, device=crow.device), (crow[1:] - crow[:-1]).long(), output_size=nnz)
    return _vals32(G[rows, col.long()])


def _check_sparse(A, name):
    if not isinstance(A, torch.Tensor) or A.layout != torch.sparse_csr or not A.is_cuda:
        raise TypeError("%s expects a CUDA/HIP torch.sparse_csr matrix" % name)
    if A.dim() != 2:
        raise ValueError("%s expects a 2-D sparse_csr matrix" % name)


class _SddmmFunction(torch.autograd.Function):
    """S = alpha * (X Y^T on A's pattern) + beta * A.  With upstream gradient G_S (on the pattern):
         dX = alpha * G_S * Y      the forward product of the cached engine, G_S's values refreshed onto it
         dY = alpha * G_S^T * X    its transposed product
         dA = beta * G_S"""

    @staticmethod
    def forward(ctx, A, X, Y, alpha, beta, fast):
        M, K = A.shape
        N = X.shape[1]
        Np = api.round_up_n(N)
        dev = A.device.index or 0
        crow, col = _index_tensors(A)
        val = A.values()
        ent = _entry_for_parts(crow, col, val, (M, K), dev, fast, values_needed=False)
        Xr, Yr = _rowmajor(X.detach(), M, N, Np), _rowmajor(Y.detach(), K, N, Np)   # (zero padding adds +0 products: the sums keep their bits)
        out = torch.empty((val.numel(),), dtype=torch.float32, device=A.device)
        if out.numel():
            vin = _vals32(val) if beta != 0.0 else None
            ent.eng.sddmm_device_rm(Np, alpha, Xr.data_ptr(), Xr.stride(0), Yr.data_ptr(), Yr.stride(0), beta,
                                    vin.data_ptr() if vin is not None else None, out.data_ptr(), torch.cuda.current_stream(A.device).cuda_stream)
        ctx.save_for_backward(crow, col, X, Y)
        ctx.shape, ctx.alpha, ctx.beta, ctx.fast, ctx.dev, ctx.vdtype = (M, K), alpha, beta, fast, dev, val.dtype
        return torch.sparse_csr_tensor(crow, col, out, size=(M, K))

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        crow, col, X, Y = ctx.saved_tensors
        M, K = ctx.shape
        N = X.shape[1]
        Np = api.round_up_n(N)
        gX = gY = gA = None
        if not any(ctx.needs_input_grad[:3]):
            return None, None, None, None, None, None
        nnz = int(col.numel())
        g = _grad_values(G, crow, col, nnz)
        stream = torch.cuda.current_stream(g.device).cuda_stream
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            eng = _entry_for_parts(crow, col, g, ctx.shape, ctx.dev, ctx.fast).eng   # the engine of the pattern, on G_S's values
            if ctx.needs_input_grad[1]:
                Yr = _rowmajor(Y.detach(), K, N, Np)
                out = torch.zeros((M, Np), dtype=torch.float32, device=g.device)
                eng.spmm_device_rm(Np, ctx.alpha, Yr.data_ptr(), Yr.stride(0), 0.0, out.data_ptr(), Np, out.data_ptr(), Np, stream)
                gX = (out if Np == N else out[:, :N]).to(X.dtype)
            if ctx.needs_input_grad[2]:
                Xr = _rowmajor(X.detach(), M, N, Np)
                out = torch.zeros((K, Np), dtype=torch.float32, device=g.device)
                eng.spmm_t_device_rm(Np, ctx.alpha, Xr.data_ptr(), Xr.stride(0), 0.0, out.data_ptr(), Np, out.data_ptr(), Np, stream)
                gY = (out if Np == N else out[:, :N]).to(Y.dtype)
        if ctx.needs_input_grad[0]:
            gA = torch.sparse_csr_tensor(crow, col, (g * ctx.beta).to(ctx.vdtype), size=(M, K))
        return gA, gX, gY, None, None, None


class _RowSoftmaxFunction(torch.autograd.Function):
    """P = softmax(scale * S) over every row's stored entries; dS = scale * P * (G - sum_row P G): both on the engine of the pattern
    (sextans_row_softmax_device, sextans_row_softmax_backward_device)."""

    @staticmethod
    def forward(ctx, S, scale, fast):
        M, K = S.shape
        dev = S.device.index or 0
        crow, col = _index_tensors(S)
        val = S.values()
        ent = _entry_for_parts(crow, col, val, (M, K), dev, fast, values_needed=False)
        x = _vals32(val)
        p = torch.empty_like(x)
        if x.numel():
            ent.eng.row_softmax_device(scale, x.data_ptr(), p.data_ptr(), torch.cuda.current_stream(S.device).cuda_stream)
        ctx.save_for_backward(crow, col, p)
        ctx.shape, ctx.scale, ctx.fast, ctx.dev, ctx.vdtype = (M, K), scale, fast, dev, val.dtype
        return torch.sparse_csr_tensor(crow, col, p.to(val.dtype), size=(M, K))

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        crow, col, p = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        g = _grad_values(G, crow, col, int(p.numel()))
        dx = torch.empty_like(p)
        if p.numel():
            ent = _entry_for_parts(crow, col, p, ctx.shape, ctx.dev, ctx.fast, values_needed=False)
            ent.eng.row_softmax_backward_device(ctx.scale, p.data_ptr(), g.data_ptr(), dx.data_ptr(), torch.cuda.current_stream(p.device).cuda_stream)
        return torch.sparse_csr_tensor(crow, col, dx.to(ctx.vdtype), size=ctx.shape), None, None


def sddmm(A, X, Y, alpha=1.0, beta=0.0, fast=False):
    """S on A's pattern, S_e = alpha * <X[r, :], Y[c, :]> + beta * A_e for every stored entry e = (r, c): a sparse_csr tensor with A's own
    index tensors and fp32 values, the bits of sextans_sddmm_device_rm (every product and sum rounded in column order).  X is (M, N),
    Y is (K, N); operands the kernel cannot read where they lie (N % 8 != 0, strides, dtype) are copied as spmm() copies them.
    Differentiable in X, Y and (beta != 0) A; the backward products run on the cached engine with the gradient's values."""
    _check_sparse(A, "sddmm")
    if not (isinstance(X, torch.Tensor) and isinstance(Y, torch.Tensor) and X.is_cuda and Y.is_cuda):
        raise TypeError("sddmm expects CUDA/HIP dense X and Y")
    M, K = A.shape
    if X.dim() != 2 or Y.dim() != 2 or X.shape[0] != M or Y.shape[0] != K or X.shape[1] != Y.shape[1] or X.shape[1] == 0:
        raise ValueError("shape mismatch")
    crow, col = _index_tensors(A)
    return _carry(_SddmmFunction.apply(A, X, Y, float(alpha), float(beta), bool(fast)), crow, col)


def row_softmax(S, scale=1.0, fast=False):
    """P on S's pattern: softmax(scale * S) over the stored entries of every row (torch.softmax's special values: -inf beside finite
    entries gives 0, an empty row nothing), a sparse_csr tensor with S's index tensors.  Computed in fp32; other value dtypes are
    converted and the result converted back.  Differentiable."""
    _check_sparse(S, "row_softmax")
    crow, col = _index_tensors(S)
    return _carry(_RowSoftmaxFunction.apply(S, float(scale), bool(fast)), crow, col)


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


def _drop_struct(p, seed, step):
    """The engine's view of (dropout, seed, step): None when nothing is dropped (the entries without dropout are then called)"""
    return api.Dropout(p, seed, step.data_ptr() if step is not None else None) if p > 0.0 else None


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
    crow, col = _index_tensors(A)
    val = A.values()
    ent = _entry_for_parts(crow, col, val, tuple(A.shape), A.device.index or 0, False, values_needed=False)
    out = torch.empty((val.numel(), heads), dtype=torch.float32, device=A.device)
    if out.numel():
        ent.eng.dropout_mask_device(heads, api.Dropout(p, int(seed), step.data_ptr() if step is not None else None), out.data_ptr(),
                                    torch.cuda.current_stream(A.device).cuda_stream)
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


class _FusedAttentionFunction(torch.autograd.Function):
    """sparse_attention(fused=True): one kernel pass forward (sextans_attention_device), a row pass and a column pass backward
    (sextans_attention_backward_device), all heads at once.  Nothing of size nnz is kept: the backward recomputes the probabilities from
    the rows' log-sum-exp.  A's values enter as an explicit bias pointer, never through the engine: no value refresh anywhere."""

    @staticmethod
    def forward(ctx, A, Q, K, V, scale, bias, fast, p=0.0, seed=0, step=None):
        M, Kk = A.shape
        H, d, dv = Q.shape[1], Q.shape[2], V.shape[2]
        dp, dvp = -(-d // 8) * 8, -(-dv // 8) * 8
        dev = A.device.index or 0
        crow, col = _index_tensors(A)
        val = A.values()
        ent = _entry_for_parts(crow, col, val, (M, Kk), dev, fast, values_needed=False)
        Qr, ldq = _heads_operand(Q.detach(), dp)
        Kr, ldk = _heads_operand(K.detach(), dp)
        Vr, ldv = _heads_operand(V.detach(), dvp)
        b = _vals32(val) if bias else None
        O = torch.empty((M, H, dvp), dtype=torch.float32, device=A.device)
        lse = torch.empty((M, H), dtype=torch.float32, device=A.device)
        args = (H, dp, dvp, scale, Qr.data_ptr(), ldq, Kr.data_ptr(), ldk, Vr.data_ptr(), ldv, b.data_ptr() if b is not None else None,
                O.data_ptr(), H * dvp, lse.data_ptr())
        drop = _drop_struct(p, seed, step)
        stream = torch.cuda.current_stream(A.device).cuda_stream
        if drop is None:
            ent.eng.attention_device(*args, stream)
        else:
            ent.eng.attention_dropout_device(*args, drop, stream)
        ctx.save_for_backward(crow, col, val, Q, K, V, O, lse)
        ctx.shape, ctx.scale, ctx.bias, ctx.fast, ctx.dev = (M, Kk), scale, bias, fast, dev
        ctx.drop = (p, seed, step)   # the backward recomputes the forward's mask
        return O if dvp == dv else O[:, :, :dv]

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        crow, col, val, Q, K, V, O, lse = ctx.saved_tensors
        M, Kk = ctx.shape
        H, d, dv = Q.shape[1], Q.shape[2], V.shape[2]
        dp, dvp = -(-d // 8) * 8, O.shape[2]
        ent = _entry_for_parts(crow, col, val, ctx.shape, ctx.dev, ctx.fast, values_needed=False)
        Qr, ldq = _heads_operand(Q.detach(), dp)
        Kr, ldk = _heads_operand(K.detach(), dp)
        Vr, ldv = _heads_operand(V.detach(), dvp)
        Gr, ldg = _heads_operand(G, dvp)           # (a copy when G has zero strides, e.g. after .sum(), or dv % 8 != 0)
        want_bias = ctx.bias and ctx.needs_input_grad[0]
        b = _vals32(val) if ctx.bias else None
        delta = torch.empty((M, H), dtype=torch.float32, device=G.device)
        dQ = torch.empty((M, H, dp), dtype=torch.float32, device=G.device)
        dK = torch.empty((Kk, H, dp), dtype=torch.float32, device=G.device)
        dV = torch.empty((Kk, H, dvp), dtype=torch.float32, device=G.device)
        db = torch.empty((val.numel(),), dtype=torch.float32, device=G.device) if want_bias else None
        args = (H, dp, dvp, ctx.scale, Qr.data_ptr(), ldq, Kr.data_ptr(), ldk, Vr.data_ptr(), ldv, b.data_ptr() if b is not None else None,
                O.data_ptr(), H * dvp, lse.data_ptr(), Gr.data_ptr(), ldg, delta.data_ptr(), dQ.data_ptr(), H * dp, dK.data_ptr(), H * dp,
                dV.data_ptr(), H * dvp, db.data_ptr() if db is not None else None)
        drop = _drop_struct(*ctx.drop)
        stream = torch.cuda.current_stream(G.device).cuda_stream
        if drop is None:
            ent.eng.attention_backward_device(*args, stream)
        else:
            ent.eng.attention_dropout_backward_device(*args, drop, stream)
        gA = torch.sparse_csr_tensor(crow, col, db.to(val.dtype), size=(M, Kk)) if want_bias else None
        gQ = (dQ if dp == d else dQ[:, :, :d]).to(Q.dtype) if ctx.needs_input_grad[1] else None
        gK = (dK if dp == d else dK[:, :, :d]).to(K.dtype) if ctx.needs_input_grad[2] else None
        gV = (dV if dvp == dv else dV[:, :, :dv]).to(V.dtype) if ctx.needs_input_grad[3] else None
        return gA, gQ, gK, gV, None, None, None, None, None, None


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


def _composed_attention(A, Q, K, V, scale, bias, fast, mult):
    """one head of the composition; mult: None, or the head's column of dropout_mask()"""
    S = sddmm(A, Q, K, 1.0, 1.0 if bias else 0.0, fast)
    P = row_softmax(S, scale, fast)
    if mult is not None:
        crow, col = _index_tensors(P)
        P = _carry(_ScaleValuesFunction.apply(P, mult), crow, col)
    return spmm(P, V, fast=fast)


def _sparse_attention(A, Q, K, V, scale, bias, fast, fused, p, seed, step):
    _check_sparse(A, "sparse_attention")
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in (Q, K, V)):
        raise TypeError("sparse_attention expects CUDA/HIP dense Q, K and V")
    if not fused and Q.dim() == 2 and K.dim() == 2 and V.dim() == 2:
        if V.shape[0] != A.shape[1]:
            raise ValueError("shape mismatch")
        if scale is None:
            scale = 1.0 / math.sqrt(Q.shape[1])
        mult = dropout_mask(A, 1, p, _draw_seed(seed), step)[:, 0] if p > 0.0 else None
        return _composed_attention(A, Q, K, V, scale, bias, fast, mult)
    if any(t.dim() not in (2, 3) for t in (Q, K, V)):
        raise ValueError("Q, K and V are (rows, d) or (rows, heads, d)")
    Q3, K3, V3 = (t if t.dim() == 3 else t.unsqueeze(1) for t in (Q, K, V))
    M, Kk = A.shape
    H, d = Q3.shape[1], Q3.shape[2]
    if K3.shape[1] != H or V3.shape[1] != H:
        raise ValueError("Q, K and V differ in their number of heads")
    if Q3.shape[0] != M or K3.shape[0] != Kk or V3.shape[0] != Kk or K3.shape[2] != d or H == 0 or d == 0 or V3.shape[2] == 0:
        raise ValueError("shape mismatch")
    if scale is None:
        scale = 1.0 / math.sqrt(d)
    if p > 0.0:
        seed, step = _draw_seed(seed), _check_step(step, A.device)
    if not fused:
        mult = dropout_mask(A, H, p, seed, step) if p > 0.0 else None
        out = torch.stack([_composed_attention(A, Q3[:, h], K3[:, h], V3[:, h], scale, bias, fast,
                                               mult[:, h].contiguous() if mult is not None else None) for h in range(H)], dim=1)
    else:
        if d > 128 or V3.shape[2] > 128:
            raise ValueError("fused sparse_attention: head dimensions up to 128")
        if p > 0.0:
            out = _FusedAttentionFunction.apply(A, Q3, K3, V3, float(scale), bool(bias), bool(fast), p, seed, step)
        else:
            out = _FusedAttentionFunction.apply(A, Q3, K3, V3, float(scale), bool(bias), bool(fast), 0.0, 0, None)
    return out if V.dim() == 3 else out[:, 0]


class _EdgeAttentionFunction(torch.autograd.Function):
    """sparse_attention_edge(): the fused attention with a key row and a value row per stored entry (sextans_attention_edge_device /
    sextans_attention_edge_backward_device).  Ek / Ev: (nnz, H, d) / (nnz, H, dv) or None; shared: Ev is Ek itself -- the backward then
    hands one buffer to the engine as both gradients and gets their sum.  As _FusedAttentionFunction: nothing of size nnz but E, dE and
    the bias, no value refresh."""

    @staticmethod
    def forward(ctx, A, Q, K, V, Ek, Ev, shared, scale, bias, fast, p, seed, step):
        M, Kk = A.shape
        H, d, dv = Q.shape[1], Q.shape[2], V.shape[2]
        dp, dvp = -(-d // 8) * 8, -(-dv // 8) * 8
        dev = A.device.index or 0
        crow, col = _index_tensors(A)
        val = A.values()
        ent = _entry_for_parts(crow, col, val, (M, Kk), dev, fast, values_needed=False)
        Qr, ldq = _heads_operand(Q.detach(), dp)
        Kr, ldk = _heads_operand(K.detach(), dp)
        Vr, ldv = _heads_operand(V.detach(), dvp)
        Ekr, ldek = _heads_operand(Ek.detach(), dp) if Ek is not None else (None, H * dp)
        Evr, ldev = (Ekr, ldek) if shared else _heads_operand(Ev.detach(), dvp) if Ev is not None else (None, H * dvp)
        b = _vals32(val) if bias else None
        O = torch.empty((M, H, dvp), dtype=torch.float32, device=A.device)
        lse = torch.empty((M, H), dtype=torch.float32, device=A.device)
        ptr = lambda t: t.data_ptr() if t is not None else None
        ent.eng.attention_edge_device(H, dp, dvp, scale, Qr.data_ptr(), ldq, Kr.data_ptr(), ldk, Vr.data_ptr(), ldv, ptr(Ekr), ldek, ptr(Evr), ldev,
                                      ptr(b), O.data_ptr(), H * dvp, lse.data_ptr(), _drop_struct(p, seed, step),
                                      torch.cuda.current_stream(A.device).cuda_stream)
        ctx.save_for_backward(crow, col, val, Q, K, V, Ek, Ev, O, lse)
        ctx.shape, ctx.scale, ctx.bias, ctx.fast, ctx.dev, ctx.shared = (M, Kk), scale, bias, fast, dev, shared
        ctx.drop = (p, seed, step)   # the backward recomputes the forward's mask
        return O if dvp == dv else O[:, :, :dv]

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        crow, col, val, Q, K, V, Ek, Ev, O, lse = ctx.saved_tensors
        M, Kk = ctx.shape
        H, d, dv = Q.shape[1], Q.shape[2], V.shape[2]
        dp, dvp = -(-d // 8) * 8, O.shape[2]
        nnz, shared = int(val.numel()), ctx.shared
        ent = _entry_for_parts(crow, col, val, ctx.shape, ctx.dev, ctx.fast, values_needed=False)
        Qr, ldq = _heads_operand(Q.detach(), dp)
        Kr, ldk = _heads_operand(K.detach(), dp)
        Vr, ldv = _heads_operand(V.detach(), dvp)
        Ekr, ldek = _heads_operand(Ek.detach(), dp) if Ek is not None else (None, H * dp)
        Evr, ldev = (Ekr, ldek) if shared else _heads_operand(Ev.detach(), dvp) if Ev is not None else (None, H * dvp)
        Gr, ldg = _heads_operand(G, dvp)
        want_bias = ctx.bias and ctx.needs_input_grad[0]
        b = _vals32(val) if ctx.bias else None
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=G.device)
        delta, dQ, dK, dV = new(M, H), new(M, H, dp), new(Kk, H, dp), new(Kk, H, dvp)
        db = new(nnz) if want_bias else None
        dEk = new(nnz, H, dp) if Ek is not None and ctx.needs_input_grad[4] else None
        dEv = dEk if shared else new(nnz, H, dvp) if Ev is not None and ctx.needs_input_grad[5] else None   # shared: ONE buffer, the sum
        ptr = lambda t: t.data_ptr() if t is not None else None
        ent.eng.attention_edge_backward_device(H, dp, dvp, ctx.scale, Qr.data_ptr(), ldq, Kr.data_ptr(), ldk, Vr.data_ptr(), ldv, ptr(Ekr), ldek,
                                               ptr(Evr), ldev, ptr(b), O.data_ptr(), H * dvp, lse.data_ptr(), Gr.data_ptr(), ldg,
                                               delta.data_ptr(), dQ.data_ptr(), H * dp, dK.data_ptr(), H * dp, dV.data_ptr(), H * dvp,
                                               ptr(dEk), H * dp, ptr(dEv), H * dvp, ptr(db), _drop_struct(*ctx.drop),
                                               torch.cuda.current_stream(G.device).cuda_stream)
        gA = torch.sparse_csr_tensor(crow, col, db.to(val.dtype), size=(M, Kk)) if want_bias else None
        gQ = (dQ if dp == d else dQ[:, :, :d]).to(Q.dtype) if ctx.needs_input_grad[1] else None
        gK = (dK if dp == d else dK[:, :, :d]).to(K.dtype) if ctx.needs_input_grad[2] else None
        gV = (dV if dvp == dv else dV[:, :, :dv]).to(V.dtype) if ctx.needs_input_grad[3] else None
        gEk = (dEk if dp == d else dEk[:, :, :d]).to(Ek.dtype) if dEk is not None else None
        gEv = (dEv if dvp == dv else dEv[:, :, :dv]).to(Ev.dtype) if dEv is not None and not shared else None
        return gA, gQ, gK, gV, gEk, gEv, None, None, None, None, None, None, None


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
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in (Q, K, V)):
        raise TypeError("sparse_attention_edge expects CUDA/HIP dense Q, K and V")
    if any(t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda) for t in (edge_key, edge_value)):
        raise TypeError("sparse_attention_edge expects CUDA/HIP dense edge_key and edge_value (or None)")
    if any(t.dim() not in (2, 3) for t in (Q, K, V)):
        raise ValueError("Q, K and V are (rows, d) or (rows, heads, d)")
    Q3, K3, V3 = (t if t.dim() == 3 else t.unsqueeze(1) for t in (Q, K, V))
    M, Kk = A.shape
    H, d, dv = Q3.shape[1], Q3.shape[2], V3.shape[2]
    if K3.shape[1] != H or V3.shape[1] != H:
        raise ValueError("Q, K and V differ in their number of heads")
    if Q3.shape[0] != M or K3.shape[0] != Kk or V3.shape[0] != Kk or K3.shape[2] != d or H == 0 or d == 0 or dv == 0:
        raise ValueError("shape mismatch")
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
    p = _check_dropout(dropout)
    if p > 0.0:
        seed, step = _draw_seed(seed), _check_step(step, A.device)
    else:
        seed, step = 0, None
    out = _EdgeAttentionFunction.apply(A, Q3, K3, V3, Ek3, Ev3, shared, float(scale), bool(bias), bool(fast), p, seed, step)
    return out if V.dim() == 3 else out[:, 0]


def _scalars_operand(t):
    """A (rows, H) tensor of per-node, per-head scalars as the GAT kernels read it: t itself where it lies that way (fp32, the heads of a
    row next to each other, rows at least H apart, 16-byte aligned base), else a contiguous fp32 copy."""
    rows, H = t.shape
    if t.dtype == torch.float32 and (H == 1 or t.stride(1) == 1) and t.stride(0) >= H and t.data_ptr() % 16 == 0:
        return t, t.stride(0)
    out = torch.empty((rows, H), dtype=torch.float32, device=t.device)
    out.copy_(t)
    return out, H


class _GatAttentionFunction(torch.autograd.Function):
    """gat_attention(): one kernel pass forward (sextans_gat_attention_device), a row pass and a column pass backward
    (sextans_gat_attention_backward_device), all heads at once.  Nothing of size nnz is kept: the backward recomputes the scores and the
    probabilities from the rows' log-sum-exp.  A's values enter as an explicit bias pointer, never through the engine: no value refresh
    anywhere."""

    @staticmethod
    def forward(ctx, A, adst, asrc, V, slope, bias, fast, p=0.0, seed=0, step=None):
        M, Kk = A.shape
        H, dv = V.shape[1], V.shape[2]
        dvp = -(-dv // 8) * 8
        dev = A.device.index or 0
        crow, col = _index_tensors(A)
        val = A.values()
        ent = _entry_for_parts(crow, col, val, (M, Kk), dev, fast, values_needed=False)
        ad, ldad = _scalars_operand(adst.detach())
        as_, ldas = _scalars_operand(asrc.detach())
        Vr, ldv = _heads_operand(V.detach(), dvp)
        b = _vals32(val) if bias else None
        O = torch.empty((M, H, dvp), dtype=torch.float32, device=A.device)
        lse = torch.empty((M, H), dtype=torch.float32, device=A.device)
        args = (H, dvp, slope, ad.data_ptr(), ldad, as_.data_ptr(), ldas, Vr.data_ptr(), ldv, b.data_ptr() if b is not None else None,
                O.data_ptr(), H * dvp, lse.data_ptr())
        drop = _drop_struct(p, seed, step)
        stream = torch.cuda.current_stream(A.device).cuda_stream
        if drop is None:
            ent.eng.gat_attention_device(*args, stream)
        else:
            ent.eng.gat_attention_dropout_device(*args, drop, stream)
        ctx.save_for_backward(crow, col, val, adst, asrc, V, O, lse)
        ctx.shape, ctx.slope, ctx.bias, ctx.fast, ctx.dev = (M, Kk), slope, bias, fast, dev
        ctx.drop = (p, seed, step)   # the backward recomputes the forward's mask
        return O if dvp == dv else O[:, :, :dv]

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        crow, col, val, adst, asrc, V, O, lse = ctx.saved_tensors
        M, Kk = ctx.shape
        H, dv = V.shape[1], V.shape[2]
        dvp = O.shape[2]
        ent = _entry_for_parts(crow, col, val, ctx.shape, ctx.dev, ctx.fast, values_needed=False)
        ad, ldad = _scalars_operand(adst.detach())
        as_, ldas = _scalars_operand(asrc.detach())
        Vr, ldv = _heads_operand(V.detach(), dvp)
        Gr, ldg = _heads_operand(G, dvp)           # (a copy when G has zero strides, e.g. after .sum(), or dv % 8 != 0)
        want_bias = ctx.bias and ctx.needs_input_grad[0]
        b = _vals32(val) if ctx.bias else None
        delta = torch.empty((M, H), dtype=torch.float32, device=G.device)
        dad = torch.empty((M, H), dtype=torch.float32, device=G.device)
        das = torch.empty((Kk, H), dtype=torch.float32, device=G.device)
        dV = torch.empty((Kk, H, dvp), dtype=torch.float32, device=G.device)
        db = torch.empty((val.numel(),), dtype=torch.float32, device=G.device) if want_bias else None
        args = (H, dvp, ctx.slope, ad.data_ptr(), ldad, as_.data_ptr(), ldas, Vr.data_ptr(), ldv, b.data_ptr() if b is not None else None,
                O.data_ptr(), H * dvp, lse.data_ptr(), Gr.data_ptr(), ldg, delta.data_ptr(), dad.data_ptr(), H, das.data_ptr(), H,
                dV.data_ptr(), H * dvp, db.data_ptr() if db is not None else None)
        drop = _drop_struct(*ctx.drop)
        stream = torch.cuda.current_stream(G.device).cuda_stream
        if drop is None:
            ent.eng.gat_attention_backward_device(*args, stream)
        else:
            ent.eng.gat_attention_dropout_backward_device(*args, drop, stream)
        gA = torch.sparse_csr_tensor(crow, col, db.to(val.dtype), size=(M, Kk)) if want_bias else None
        gad = dad.to(adst.dtype) if ctx.needs_input_grad[1] else None
        gas = das.to(asrc.dtype) if ctx.needs_input_grad[2] else None
        gV = (dV if dvp == dv else dV[:, :, :dv]).to(V.dtype) if ctx.needs_input_grad[3] else None
        return gA, gad, gas, gV, None, None, None, None, None, None


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
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in (a_dst, a_src, V)):
        raise TypeError("gat_attention expects CUDA/HIP dense a_dst, a_src and V")
    if V.dim() not in (2, 3) or a_dst.dim() not in (1, 2) or a_src.dim() not in (1, 2):
        raise ValueError("a_dst and a_src are (rows,) or (rows, heads), V is (rows, dv) or (rows, heads, dv)")
    V3 = V if V.dim() == 3 else V.unsqueeze(1)
    ad2 = a_dst if a_dst.dim() == 2 else a_dst.unsqueeze(1)
    as2 = a_src if a_src.dim() == 2 else a_src.unsqueeze(1)
    M, Kk = A.shape
    H, dv = V3.shape[1], V3.shape[2]
    if ad2.shape[1] != H or as2.shape[1] != H:
        raise ValueError("a_dst, a_src and V differ in their number of heads")
    if ad2.shape[0] != M or as2.shape[0] != Kk or V3.shape[0] != Kk or H == 0 or dv == 0:
        raise ValueError("shape mismatch")
    if dv > 128:
        raise ValueError("gat_attention: dv up to 128")
    slope = float(negative_slope)
    if not (slope >= 0.0) or math.isinf(slope):
        raise ValueError("negative_slope must be finite and >= 0")
    if p > 0.0:
        out = _GatAttentionFunction.apply(A, ad2, as2, V3, slope, bool(bias), bool(fast), p, _draw_seed(seed), _check_step(step, A.device))
    else:
        out = _GatAttentionFunction.apply(A, ad2, as2, V3, slope, bool(bias), bool(fast), 0.0, 0, None)
    return out if V.dim() == 3 else out[:, 0]


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
        dvp = -(-dv // 8) * 8
        dev = A.device.index or 0
        soft = mode == api.SCORE_SOFTMAX
        crow, col = _index_tensors(A)
        val = A.values()
        ent = _entry_for_parts(crow, col, val, (M, Kk), dev, fast, values_needed=False)
        Sr, lds = _scalars_operand(S.detach())
        Vr, ldv = _heads_operand(V.detach(), dvp)
        O = torch.empty((M, H, dvp), dtype=torch.float32, device=A.device)
        lse = torch.empty((M, H) if soft else (0,), dtype=torch.float32, device=A.device)
        ent.eng.score_attention_device(mode, H, dvp, Sr.data_ptr(), lds, Vr.data_ptr(), ldv, O.data_ptr(), H * dvp,
                                       lse.data_ptr() if soft else None, _drop_struct(p, seed, step),
                                       torch.cuda.current_stream(A.device).cuda_stream)
        ctx.save_for_backward(crow, col, val, S, V, *((O, lse) if soft else ()))
        ctx.shape, ctx.mode, ctx.fast, ctx.dev, ctx.dvp = (M, Kk), mode, fast, dev, dvp
        ctx.drop = (p, seed, step)   # the backward recomputes the forward's mask
        ctx.mark_non_differentiable(lse)
        return (O if dvp == dv else O[:, :, :dv]), lse

    @staticmethod
    @once_differentiable
    def backward(ctx, G, _):
        crow, col, val, S, V = ctx.saved_tensors[:5]
        soft = ctx.mode == api.SCORE_SOFTMAX
        O, lse = ctx.saved_tensors[5:] if soft else (None, None)
        M, Kk = ctx.shape
        H, dv = V.shape[1], V.shape[2]
        dvp = ctx.dvp
        ent = _entry_for_parts(crow, col, val, ctx.shape, ctx.dev, ctx.fast, values_needed=False)
        Sr, lds = _scalars_operand(S.detach())
        Vr, ldv = _heads_operand(V.detach(), dvp)
        Gr, ldg = _heads_operand(G, dvp)           # (a copy when G has zero strides, e.g. after .sum(), or dv % 8 != 0)
        dS = torch.empty((S.shape[0], H), dtype=torch.float32, device=G.device) if ctx.needs_input_grad[1] else None
        dV = torch.empty((Kk, H, dvp), dtype=torch.float32, device=G.device) if ctx.needs_input_grad[2] else None
        ent.eng.score_attention_backward_device(ctx.mode, H, dvp, Sr.data_ptr(), lds, Vr.data_ptr(), ldv, O.data_ptr() if soft else None, H * dvp,
                                                lse.data_ptr() if soft else None, Gr.data_ptr(), ldg,
                                                dS.data_ptr() if dS is not None else None, H, dV.data_ptr() if dV is not None else None, H * dvp,
                                                _drop_struct(*ctx.drop), torch.cuda.current_stream(G.device).cuda_stream)
        gS = dS.to(S.dtype) if dS is not None else None
        gV = (dV if dvp == dv else dV[:, :, :dv]).to(V.dtype) if dV is not None else None
        return None, gS, gV, None, None, None, None, None


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
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in (S, V)):
        raise TypeError("score_attention expects CUDA/HIP dense S and V")
    if V.dim() not in (2, 3) or S.dim() not in (1, 2):
        raise ValueError("S is (nnz,) or (nnz, heads), V is (rows, dv) or (rows, heads, dv)")
    V3 = V if V.dim() == 3 else V.unsqueeze(1)
    S2 = S if S.dim() == 2 else S.unsqueeze(1)
    M, Kk = A.shape
    H, dv = V3.shape[1], V3.shape[2]
    if S2.shape[1] != H:
        raise ValueError("S and V differ in their number of heads")
    if S2.shape[0] != A.values().numel() or V3.shape[0] != Kk or H == 0 or dv == 0:
        raise ValueError("shape mismatch")
    if dv > 128:
        raise ValueError("score_attention: dv up to 128")
    p = _check_dropout(dropout)
    soft = mode == api.SCORE_SOFTMAX
    if not soft and (p > 0.0 or return_weights):
        raise ValueError("normalize='none': the caller holds the weights (no dropout, no return_weights)")
    if p > 0.0:
        out, lse = _ScoreAttentionFunction.apply(A, S2, V3, mode, bool(fast), p, _draw_seed(seed), _check_step(step, A.device))
    else:
        out, lse = _ScoreAttentionFunction.apply(A, S2, V3, mode, bool(fast), 0.0, 0, None)
    out = out if V.dim() == 3 else out[:, 0]
    if not return_weights:
        return out
    w = torch.exp(S2.detach().to(torch.float32) - lse[entry_rows(A)])
    return out, (w if S.dim() == 2 else w[:, 0])


class _Gatv2AttentionFunction(torch.autograd.Function):
    """gatv2_attention(): one kernel pass forward (sextans_gatv2_attention_device), a row pass, a column pass and the two-level datt sum
    backward (sextans_gatv2_attention_backward_device), all heads at once.  Nothing of size nnz is kept: the backward recomputes the
    scores and the probabilities from the rows' log-sum-exp.  A's values enter as an explicit bias pointer: no value refresh anywhere.
    x_dst and x_src may be the same tensor: autograd adds the two gradients."""

    @staticmethod
    def forward(ctx, A, xdst, xsrc, att, slope, bias, fast, p=0.0, seed=0, step=None):
        M, Kk = A.shape
        H, d = xdst.shape[1], xdst.shape[2]
        dp = -(-d // 8) * 8
        dev = A.device.index or 0
        crow, col = _index_tensors(A)
        val = A.values()
        ent = _entry_for_parts(crow, col, val, (M, Kk), dev, fast, values_needed=False)
        xd, ldxd = _heads_operand(xdst.detach(), dp)
        xs, ldxs = _heads_operand(xsrc.detach(), dp)
        at, _ = _heads_operand(att.detach().unsqueeze(0), dp)      # (1, H, dp): heads * dp floats, contiguous
        b = _vals32(val) if bias else None
        O = torch.empty((M, H, dp), dtype=torch.float32, device=A.device)
        lse = torch.empty((M, H), dtype=torch.float32, device=A.device)
        args = (H, dp, slope, xd.data_ptr(), ldxd, xs.data_ptr(), ldxs, at.data_ptr(), b.data_ptr() if b is not None else None, O.data_ptr(),
                H * dp, lse.data_ptr())
        drop = _drop_struct(p, seed, step)
        stream = torch.cuda.current_stream(A.device).cuda_stream
        if drop is None:
            ent.eng.gatv2_attention_device(*args, stream)
        else:
            ent.eng.gatv2_attention_dropout_device(*args, drop, stream)
        ctx.save_for_backward(crow, col, val, xdst, xsrc, att, O, lse)
        ctx.shape, ctx.slope, ctx.bias, ctx.fast, ctx.dev = (M, Kk), slope, bias, fast, dev
        ctx.drop = (p, seed, step)   # the backward recomputes the forward's mask
        return O if dp == d else O[:, :, :d]

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        crow, col, val, xdst, xsrc, att, O, lse = ctx.saved_tensors
        M, Kk = ctx.shape
        H, d = xdst.shape[1], xdst.shape[2]
        dp = O.shape[2]
        ent = _entry_for_parts(crow, col, val, ctx.shape, ctx.dev, ctx.fast, values_needed=False)
        xd, ldxd = _heads_operand(xdst.detach(), dp)
        xs, ldxs = _heads_operand(xsrc.detach(), dp)
        at, _ = _heads_operand(att.detach().unsqueeze(0), dp)
        Gr, ldg = _heads_operand(G, dp)           # (a copy when G has zero strides, e.g. after .sum(), or d % 8 != 0)
        want_bias = ctx.bias and ctx.needs_input_grad[0]
        b = _vals32(val) if ctx.bias else None
        delta = torch.empty((M, H), dtype=torch.float32, device=G.device)
        dxd = torch.empty((M, H, dp), dtype=torch.float32, device=G.device)
        dxs = torch.empty((Kk, H, dp), dtype=torch.float32, device=G.device)
        dat = torch.empty((H, dp), dtype=torch.float32, device=G.device)
        work = torch.empty((max(ent.eng.gatv2_workspace_floats(H, dp), 1),), dtype=torch.float32, device=G.device)
        db = torch.empty((val.numel(),), dtype=torch.float32, device=G.device) if want_bias else None
        args = (H, dp, ctx.slope, xd.data_ptr(), ldxd, xs.data_ptr(), ldxs, at.data_ptr(), b.data_ptr() if b is not None else None,
                O.data_ptr(), H * dp, lse.data_ptr(), Gr.data_ptr(), ldg, delta.data_ptr(), dxd.data_ptr(), H * dp, dxs.data_ptr(), H * dp,
                dat.data_ptr(), work.data_ptr(), db.data_ptr() if db is not None else None)
        drop = _drop_struct(*ctx.drop)
        stream = torch.cuda.current_stream(G.device).cuda_stream
        if drop is None:
            ent.eng.gatv2_attention_backward_device(*args, stream)
        else:
            ent.eng.gatv2_attention_dropout_backward_device(*args, drop, stream)
        gA = torch.sparse_csr_tensor(crow, col, db.to(val.dtype), size=(M, Kk)) if want_bias else None
        gxd = (dxd if dp == d else dxd[:, :, :d]).to(xdst.dtype) if ctx.needs_input_grad[1] else None
        gxs = (dxs if dp == d else dxs[:, :, :d]).to(xsrc.dtype) if ctx.needs_input_grad[2] else None
        gat = (dat if dp == d else dat[:, :d]).to(att.dtype) if ctx.needs_input_grad[3] else None
        return gA, gxd, gxs, gat, None, None, None, None, None, None


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
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in (x_dst, x_src, att)):
        raise TypeError("gatv2_attention expects CUDA/HIP dense x_dst, x_src and att")
    if x_dst.dim() not in (2, 3) or x_src.dim() != x_dst.dim() or att.dim() != x_dst.dim() - 1:
        raise ValueError("x_dst, x_src and att are (rows, heads, d), (rows, heads, d) and (heads, d), or (rows, d), (rows, d) and (d,)")
    xd3, xs3, at2 = (x_dst, x_src, att) if x_dst.dim() == 3 else (x_dst.unsqueeze(1), x_src.unsqueeze(1), att.unsqueeze(0))
    M, Kk = A.shape
    H, d = xd3.shape[1], xd3.shape[2]
    if xs3.shape[1] != H or at2.shape[0] != H:
        raise ValueError("x_dst, x_src and att differ in their number of heads")
    if xd3.shape[0] != M or xs3.shape[0] != Kk or xs3.shape[2] != d or at2.shape[1] != d or H == 0 or d == 0:
        raise ValueError("shape mismatch")
    if d > 128:
        raise ValueError("gatv2_attention: d up to 128")
    slope = float(negative_slope)
    if not (slope >= 0.0) or math.isinf(slope):
        raise ValueError("negative_slope must be finite and >= 0")
    if p > 0.0:
        out = _Gatv2AttentionFunction.apply(A, xd3, xs3, at2, slope, bool(bias), bool(fast), p, _draw_seed(seed), _check_step(step, A.device))
    else:
        out = _Gatv2AttentionFunction.apply(A, xd3, xs3, at2, slope, bool(bias), bool(fast), 0.0, 0, None)
    return out if x_dst.dim() == 3 else out[:, 0]


_REDUCE_OPS = {"amax": api.REDUCE_MAX, "amin": api.REDUCE_MIN}


def _reduce_forward(A, B, op, fast, want_arg):
    """(C, arg) of the engine's max / min aggregation, both (M, Np) with N padded up to a multiple of 8 (zero columns of B); arg is None
    unless asked for."""
    M, K = A.shape
    N = B.shape[1]
    Np = api.round_up_n(N)
    crow, col = _index_tensors(A)
    val = A.values()
    ent = _entry_for_parts(crow, col, val, (M, K), A.device.index or 0, fast, values_needed=False)
    Brm = _rowmajor(B.detach(), K, N, Np)
    v = _vals32(val)
    C = torch.empty((M, Np), dtype=torch.float32, device=A.device)
    arg = torch.empty((M, Np), dtype=torch.int32, device=A.device) if want_arg else None
    ent.eng.spmm_reduce_device_rm(op, Np, v.data_ptr() if v.numel() else None, Brm.data_ptr() if Brm.numel() else None, Brm.stride(0),
                                  C.data_ptr() if C.numel() else None, Np, arg.data_ptr() if arg is not None and arg.numel() else None, Np,
                                  torch.cuda.current_stream(A.device).cuda_stream)
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
        ctx.shape, ctx.fast, ctx.dev = tuple(A.shape), fast, A.device.index or 0
        out_arg = arg if arg.shape[1] == N else arg[:, :N]
        ctx.mark_non_differentiable(out_arg)
        return (C if C.shape[1] == N else C[:, :N]), out_arg

    @staticmethod
    @once_differentiable
    def backward(ctx, G, _):
        crow, col, val, B, arg = ctx.saved_tensors
        M, K = ctx.shape
        N = B.shape[1]
        Np = arg.shape[1]
        want_a, want_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_a or want_b):
            return None, None, None, None
        ent = _entry_for_parts(crow, col, val, ctx.shape, ctx.dev, ctx.fast, values_needed=False)
        Grm = _rowmajor(G, M, N, Np)               # (a copy when G has zero strides, e.g. after .sum(), or N % 8 != 0)
        Brm = _rowmajor(B.detach(), K, N, Np) if want_a else None
        v = _vals32(val)
        dB = torch.empty((K, Np), dtype=torch.float32, device=G.device) if want_b else None
        dv = torch.empty((val.numel(),), dtype=torch.float32, device=G.device) if want_a else None
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        if ptr(dB) is not None or ptr(dv) is not None:   # (else: no element to write)
            ent.eng.spmm_reduce_backward_device_rm(Np, ptr(v), ptr(Brm), Brm.stride(0) if Brm is not None else Np, ptr(arg), Np, ptr(Grm),
                                                   Grm.stride(0), ptr(dB), Np, ptr(dv), torch.cuda.current_stream(G.device).cuda_stream)
        gA = torch.sparse_csr_tensor(crow, col, dv.to(val.dtype), size=(M, K)) if want_a else None
        gB = (dB if Np == N else dB[:, :N]).to(B.dtype) if want_b else None
        return gA, gB, None, None


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
        crow = _index_tensors(A)[0]
        out = spmm(A, B, fast=fast)
        return out / (crow[1:] - crow[:-1]).clamp(min=1).to(out.dtype)[:, None]
    _check_sparse(A, "spmm_reduce")
    if not (isinstance(B, torch.Tensor) and B.is_cuda):
        raise TypeError("spmm_reduce expects a CUDA/HIP dense B")
    if B.dim() != 2 or B.shape[0] != A.shape[1] or B.shape[1] == 0:
        raise ValueError("shape mismatch")
    op = _REDUCE_OPS[reduce]
    if torch.is_grad_enabled() and (A.requires_grad or B.requires_grad):
        C, arg = _SpmmReduceFunction.apply(A, B, op, bool(fast))
    else:
        C, arg = _reduce_forward(A, B, op, bool(fast), bool(return_arg))
        N = B.shape[1]
        if C.shape[1] != N:
            C, arg = C[:, :N], (arg[:, :N] if arg is not None else None)
    return (C, arg) if return_arg else C


def _softagg_forward(A, B, t, fast, want_lse):
    """(C, lse, tp) of the engine's softmax aggregation: C and lse (M, Np) with N padded up to a multiple of 8 (zero columns of B), lse
    None unless asked for; tp the (Np,) fp32 temperatures handed to the kernel (padded columns: 1), None for t = 1 everywhere."""
    M, K = A.shape
    N = B.shape[1]
    Np = api.round_up_n(N)
    crow, col = _index_tensors(A)
    val = A.values()
    ent = _entry_for_parts(crow, col, val, (M, K), A.device.index or 0, fast, values_needed=False)
    Brm = _rowmajor(B.detach(), K, N, Np)
    v = _vals32(val)
    tp = None
    if t is not None:
        tp = torch.ones((Np,), dtype=torch.float32, device=A.device)
        tp[:N] = t.detach()
    C = torch.empty((M, Np), dtype=torch.float32, device=A.device)
    lse = torch.empty((M, Np), dtype=torch.float32, device=A.device) if want_lse else None
    ent.eng.spmm_softagg_device_rm(Np, v.data_ptr() if v.numel() else None, Brm.data_ptr() if Brm.numel() else None, Brm.stride(0),
                                   tp.data_ptr() if tp is not None else None, C.data_ptr() if C.numel() else None, Np,
                                   lse.data_ptr() if lse is not None and lse.numel() else None, Np,
                                   torch.cuda.current_stream(A.device).cuda_stream)
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
        ctx.shape, ctx.fast, ctx.dev = tuple(A.shape), fast, A.device.index or 0
        ctx.t_dtype = t.dtype if t is not None else None
        out_lse = lse if lse.shape[1] == N else lse[:, :N]
        ctx.mark_non_differentiable(out_lse)
        return (C if C.shape[1] == N else C[:, :N]), out_lse

    @staticmethod
    @once_differentiable
    def backward(ctx, G, _):
        crow, col, val, B, C, lse = ctx.saved_tensors[:6]
        tp = ctx.saved_tensors[6] if len(ctx.saved_tensors) > 6 else None
        M, K = ctx.shape
        N = B.shape[1]
        Np = C.shape[1]
        want_a, want_b, want_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1], tp is not None and ctx.needs_input_grad[2]
        if not (want_a or want_b or want_t):
            return None, None, None, None
        ent = _entry_for_parts(crow, col, val, ctx.shape, ctx.dev, ctx.fast, values_needed=False)
        Grm = _rowmajor(G, M, N, Np)               # (a copy when G has zero strides, e.g. after .sum(), or N % 8 != 0)
        Brm = _rowmajor(B.detach(), K, N, Np)
        v = _vals32(val)
        dB = torch.empty((K, Np), dtype=torch.float32, device=G.device) if want_b else None
        dv = torch.empty((val.numel(),), dtype=torch.float32, device=G.device) if want_a else None
        dt = torch.empty((Np,), dtype=torch.float32, device=G.device) if want_t else None
        work = torch.empty((max(ent.eng.spmm_softagg_workspace_floats(Np), 1),), dtype=torch.float32, device=G.device) if want_t else None
        ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
        if ptr(dB) is not None or ptr(dv) is not None or dt is not None:   # (else: no element to write)
            ent.eng.spmm_softagg_backward_device_rm(Np, ptr(v), ptr(Brm), Brm.stride(0), ptr(tp), ptr(C), Np, ptr(lse), Np, ptr(Grm),
                                                    Grm.stride(0), ptr(dB), Np, ptr(dv), ptr(dt), ptr(work),
                                                    torch.cuda.current_stream(G.device).cuda_stream)
        gA = torch.sparse_csr_tensor(crow, col, dv.to(val.dtype), size=(M, K)) if want_a else None
        gB = (dB if Np == N else dB[:, :N]).to(B.dtype) if want_b else None
        gt = (dt if Np == N else dt[:N]).to(ctx.t_dtype) if want_t else None
        return gA, gB, gt, None


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
    if not (isinstance(B, torch.Tensor) and B.is_cuda):
        raise TypeError("spmm_softagg expects a CUDA/HIP dense B")
    if B.dim() != 2 or B.shape[0] != A.shape[1] or B.shape[1] == 0:
        raise ValueError("shape mismatch")
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
        C, lse, _ = _softagg_forward(A, B, tv, bool(fast), bool(return_lse))
        if C.shape[1] != N:
            C, lse = C[:, :N], (lse[:, :N] if lse is not None else None)
    return (C, lse) if return_lse else C


_MULTI_RAW = ("sum", "sumsq", "max", "min")                       # what the kernel computes, in the order of sextans_multi_out
_MULTI_NEEDS = {"sum": ("sum",), "mean": ("sum",), "max": ("max",), "min": ("min",), "sumsq": ("sumsq",),
                "var": ("sum", "sumsq"), "std": ("sum", "sumsq")}   # aggregate -> the raw aggregates it is made of


def _multi_raw(A, B, want, place, width, fast, want_arg, E=None, op=None):
    """One forward call of the engine's multi-aggregation.  want: the raw aggregates to compute; place: raw name -> the index of its
    N-column block in an (M, width) output that the kernel writes in place (N % 8 == 0 only; empty: no such output).
    -> (out or None, {raw name not placed: (M, Np) tensor}, argmax, argmin), Np = N padded up to a multiple of 8.
    E (nnz, N) and op (EDGE_*): the edge-feature messages of spmm_edge_multi() instead of A_e * B[c] (B is None for EDGE_COPY)."""
    M, K = A.shape
    N = (B if E is None else E).shape[1]
    Np = api.round_up_n(N)
    crow, col = _index_tensors(A)
    val = A.values()
    ent = _entry_for_parts(crow, col, val, (M, K), A.device.index or 0, fast, values_needed=False)
    Brm = _rowmajor(B.detach(), K, N, Np) if B is not None else None
    v = _vals32(val) if E is None else None
    out = torch.empty((M, width), dtype=torch.float32, device=A.device) if place else None
    tmp = {name: torch.empty((M, Np), dtype=torch.float32, device=A.device) for name in want if name not in place}
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
        o.d_argmax, o.d_argmin = (t.data_ptr() if t is not None else None for t in args)
        o.ld_arg = Np
        stream = torch.cuda.current_stream(A.device).cuda_stream
        if E is None:
            ent.eng.spmm_multi_device_rm(Np, v.data_ptr() if v.numel() else None, Brm.data_ptr() if Brm.numel() else None, Brm.stride(0), o, stream)
        else:
            Erm = _rowmajor(E.detach(), E.shape[0], N, Np)
            ent.eng.spmm_edge_multi_device_rm(op, Np, Brm.data_ptr() if Brm is not None and Brm.numel() else None,
                                              Brm.stride(0) if Brm is not None else Np, Erm.data_ptr() if Erm.numel() else None, Erm.stride(0), o,
                                              stream)
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
    """spmm_multi(): ONE forward call (sextans_spmm_multi_device_rm) for the raw aggregates that are needed and the args of the extrema,
    ONE backward call (sextans_spmm_multi_backward_device_rm) that takes the upstream gradients that exist -- a column pass over A^T for
    dB and a row pass over A for dA, each only when autograd asks for it.  A's values enter as an explicit pointer, never through the
    engine: no value refresh anywhere.  Outputs: the (M, width) tensor with the raw aggregates written in place (or None), then sum,
    sumsq, max, min as tensors of their own where they are not placed (else None), argmax, argmin.  Not twice differentiable."""

    @staticmethod
    def forward(ctx, A, B, want, place, width, fast):
        N = B.shape[1]
        out, tmp, amax, amin = _multi_raw(A, B, want, place, width, fast, True)
        ctx.save_for_backward(*_index_tensors(A), A.values(), B, *(t for t in (amax, amin) if t is not None))
        ctx.shape, ctx.fast, ctx.dev, ctx.want, ctx.place = tuple(A.shape), fast, A.device.index or 0, want, place
        ctx.set_materialize_grads(False)
        cut = lambda t: t if t is None or t.shape[1] == N else t[:, :N]
        amax, amin = cut(amax), cut(amin)
        ctx.mark_non_differentiable(*(t for t in (amax, amin) if t is not None))
        return (out,) + tuple(cut(tmp.get(name)) for name in _MULTI_RAW) + (amax, amin)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, *g_raw):
        crow, col, val, B, *args = ctx.saved_tensors
        M, K = ctx.shape
        N = B.shape[1]
        Np = api.round_up_n(N)
        want_a, want_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        none = (None,) * 6
        if not (want_a or want_b):
            return none
        g, keep, given = _multi_grads(ctx, g_out, g_raw, args, M, N, Np)   # (keep: alive over the call)
        Brm = _rowmajor(B.detach(), K, N, Np) if (want_a or g.d_gsumsq) else None
        v = _vals32(val)
        new = torch.empty if given else torch.zeros   # (no upstream gradient at all: zeros, no call)
        dB = new((K, Np), dtype=torch.float32, device=val.device) if want_b else None
        dv = new((val.numel(),), dtype=torch.float32, device=val.device) if want_a else None
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        if given and M and (ptr(dB) is not None or ptr(dv) is not None):   # (else: no element to write)
            ctx_eng = _entry_for_parts(crow, col, val, ctx.shape, ctx.dev, ctx.fast, values_needed=False).eng
            ctx_eng.spmm_multi_backward_device_rm(Np, ptr(v), ptr(Brm), Brm.stride(0) if Brm is not None else Np, g, ptr(dB), Np, ptr(dv),
                                                  torch.cuda.current_stream(val.device).cuda_stream)
        elif given:
            for t in (dB, dv):
                if t is not None:
                    t.zero_()
        gA = torch.sparse_csr_tensor(crow, col, dv.to(val.dtype), size=(M, K)) if want_a else None
        gB = (dB if Np == N else dB[:, :N]).to(B.dtype) if want_b else None
        return (gA, gB) + none[2:]


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
    if not (isinstance(B, torch.Tensor) and B.is_cuda):
        raise TypeError("spmm_multi expects a CUDA/HIP dense B")
    if B.dim() != 2 or B.shape[0] != A.shape[1] or B.shape[1] == 0:
        raise ValueError("shape mismatch")
    N = B.shape[1]
    want, place, width = _multi_plan(aggr, N)
    if torch.is_grad_enabled() and (A.requires_grad or B.requires_grad):
        out, *raw = _SpmmMultiFunction.apply(A, B, want, place, width, bool(fast))[:5]
        raw = dict(zip(_MULTI_RAW, raw))
    else:
        out, raw, _, _ = _multi_raw(A, B, want, place, width, bool(fast), False)
        raw = {name: (t if t.shape[1] == N else t[:, :N]) for name, t in raw.items()}
    return _multi_finish(A, aggr, out, raw, place, N, eps)


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


def _multi_finish(A, aggr, out, raw, place, N, eps):
    """The result of spmm_multi() / spmm_edge_multi() from the kernel's raw aggregates: the derived ones on top, side by side in aggr's order."""
    for name, j in place.items():
        raw[name] = out[:, j * N:(j + 1) * N]
    got = dict(raw)   # every aggregate that is asked for or needed on the way, from the raw ones
    if any(name in aggr for name in ("mean", "var", "std")):
        crow = _index_tensors(A)[0]
        deg = (crow[1:] - crow[:-1]).clamp(min=1).to(torch.float32)[:, None]
        got["mean"] = raw["sum"] / deg
        if "var" in aggr or "std" in aggr:
            got["var"] = raw["sumsq"] / deg - got["mean"] ** 2
        if "std" in aggr:
            got["std"] = torch.sqrt(torch.relu(got["var"]) + eps)
    if out is None:
        return torch.cat([got[name] for name in aggr], dim=1)
    blocks = tuple(j for j, name in enumerate(aggr) if name not in place)
    return _MultiAssemble.apply(out, blocks, *(got[aggr[j]] for j in blocks)) if blocks else out


_EDGE_OPS = {"mul": api.EDGE_MUL, "add": api.EDGE_ADD, "add_relu": api.EDGE_ADD_RELU, "copy": api.EDGE_COPY}


def _edge_forward(A, B, E, op, fast):
    """C (M, Np) of the engine's edge-feature SpMM, N padded up to a multiple of 8 (zero columns of B and E); B is None for EDGE_COPY."""
    M, K = A.shape
    nnz, N = E.shape
    Np = api.round_up_n(N)
    crow, col = _index_tensors(A)
    ent = _entry_for_parts(crow, col, A.values(), (M, K), A.device.index or 0, fast, values_needed=False)
    Brm = _rowmajor(B.detach(), K, N, Np) if B is not None else None
    Erm = _rowmajor(E.detach(), nnz, N, Np)
    C = torch.empty((M, Np), dtype=torch.float32, device=A.device)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    if C.numel():
        ent.eng.spmm_edge_device_rm(op, Np, ptr(Brm), Brm.stride(0) if Brm is not None else Np, ptr(Erm), Erm.stride(0), ptr(C), Np,
                                    torch.cuda.current_stream(A.device).cuda_stream)
    return C


class _SpmmEdgeFunction(torch.autograd.Function):
    """spmm_edge(): one kernel pass forward (sextans_spmm_edge_device_rm); backward a column pass over A^T for dB and a row pass over A
    that stores dE (sextans_spmm_edge_backward_device_rm).  Only the gradients autograd asks for are computed, and only the operands
    their formulas read are handed over.  A's values never enter: no gradient for A, no value refresh.  Not twice differentiable."""

    @staticmethod
    def forward(ctx, A, B, E, op, fast):
        N = E.shape[1]
        C = _edge_forward(A, B, E, op, fast)
        ctx.save_for_backward(*_index_tensors(A), A.values(), B, E)
        ctx.shape, ctx.op, ctx.fast, ctx.dev = tuple(A.shape), op, fast, A.device.index or 0
        return C if C.shape[1] == N else C[:, :N]

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
        ent = _entry_for_parts(crow, col, val, ctx.shape, ctx.dev, ctx.fast, values_needed=False)
        need_b = op == api.EDGE_ADD_RELU or (op == api.EDGE_MUL and want_e)
        need_e = op == api.EDGE_ADD_RELU or (op == api.EDGE_MUL and want_b)
        Grm = _rowmajor(G, M, N, Np)               # (a copy when G has zero strides, e.g. after .sum(), or N % 8 != 0)
        Brm = _rowmajor(B.detach(), K, N, Np) if need_b else None
        Erm = _rowmajor(E.detach(), nnz, N, Np) if need_e else None
        dB = torch.empty((K, Np), dtype=torch.float32, device=G.device) if want_b else None
        dE = torch.empty((nnz, Np), dtype=torch.float32, device=G.device) if want_e else None
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        if ptr(dB) is not None or ptr(dE) is not None:   # (else: no element to write)
            ent.eng.spmm_edge_backward_device_rm(op, Np, ptr(Brm), Brm.stride(0) if Brm is not None else Np, ptr(Erm),
                                                 Erm.stride(0) if Erm is not None else Np, ptr(Grm), Grm.stride(0), ptr(dB), Np, ptr(dE), Np,
                                                 torch.cuda.current_stream(G.device).cuda_stream)
        gB = (dB if Np == N else dB[:, :N]).to(B.dtype) if want_b else None
        gE = (dE if Np == N else dE[:, :N]).to(E.dtype) if want_e else None
        return None, gB, gE, None, None


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
    operands the kernel cannot read where they lie, are copied with zero padding, as spmm() does."""
    if op not in _EDGE_OPS:
        raise ValueError("op must be 'mul', 'add', 'add_relu' or 'copy'")
    if reduce not in ("sum", "mean"):
        raise ValueError("reduce must be 'sum' or 'mean'")
    _check_sparse(A, "spmm_edge")
    if (B is None) != (op == "copy"):
        raise ValueError("spmm_edge: B=None goes with op='copy', and only with it")
    if not (isinstance(E, torch.Tensor) and E.is_cuda and (B is None or (isinstance(B, torch.Tensor) and B.is_cuda))):
        raise TypeError("spmm_edge expects CUDA/HIP dense B and E")
    if E.dim() not in (2, 3) or (B is not None and (B.dim() != E.dim() or B.shape[1:] != E.shape[1:])):
        raise ValueError("spmm_edge: B is (K, N) or (K, H, d), E (nnz, N) or (nnz, H, d) with the same trailing shape")
    M, K = A.shape
    if E.shape[0] != A.values().numel() or (B is not None and B.shape[0] != K) or 0 in E.shape[1:]:
        raise ValueError("shape mismatch")
    tail = tuple(E.shape[1:])
    B2 = B.reshape(K, math.prod(tail)) if B is not None else None
    E2 = E.reshape(E.shape[0], math.prod(tail))
    code = _EDGE_OPS[op]
    if torch.is_grad_enabled() and ((B2 is not None and B2.requires_grad) or E2.requires_grad):
        out = _SpmmEdgeFunction.apply(A, B2, E2, code, bool(fast))
    else:
        out = _edge_forward(A, B2, E2, code, bool(fast))
        if out.shape[1] != E2.shape[1]:
            out = out[:, :E2.shape[1]]
    if reduce == "mean":
        crow = _index_tensors(A)[0]
        out = out / (crow[1:] - crow[:-1]).clamp(min=1).to(out.dtype)[:, None]
    return out.reshape((M,) + tail)


class _SpmmEdgeMultiFunction(torch.autograd.Function):
    """spmm_edge_multi() / spmm_edge_reduce(): ONE forward call (sextans_spmm_edge_multi_device_rm) for the raw aggregates that are
    needed and the args of the extrema, ONE backward call (sextans_spmm_edge_multi_backward_device_rm) that takes the upstream gradients
    that exist -- a column pass over A^T for dB, a row pass over A that stores dE, each only when autograd asks for it.  A's values never
    enter: no gradient for A, no value refresh.  Outputs as _SpmmMultiFunction's.  Not twice differentiable."""

    @staticmethod
    def forward(ctx, A, B, E, op, want, place, width, fast):
        N = E.shape[1]
        out, tmp, amax, amin = _multi_raw(A, B, want, place, width, fast, True, E, op)
        ctx.save_for_backward(*_index_tensors(A), A.values(), B, E, *(t for t in (amax, amin) if t is not None))
        ctx.shape, ctx.op, ctx.fast, ctx.dev, ctx.want, ctx.place = tuple(A.shape), op, fast, A.device.index or 0, want, place
        ctx.set_materialize_grads(False)
        cut = lambda t: t if t is None or t.shape[1] == N else t[:, :N]
        amax, amin = cut(amax), cut(amin)
        ctx.mark_non_differentiable(*(t for t in (amax, amin) if t is not None))
        return (out,) + tuple(cut(tmp.get(name)) for name in _MULTI_RAW) + (amax, amin)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, *g_raw):
        crow, col, val, B, E, *args = ctx.saved_tensors
        M, K = ctx.shape
        nnz, N = E.shape
        Np = api.round_up_n(N)
        want_b, want_e = B is not None and ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        none = (None,) * 8
        if not (want_b or want_e):
            return none
        g, keep, given = _multi_grads(ctx, g_out, g_raw, args, M, N, Np)   # (keep: alive over the call)
        new = torch.empty if given else torch.zeros   # (no upstream gradient at all: zeros, no call)
        dB = new((K, Np), dtype=torch.float32, device=E.device) if want_b else None
        dE = new((nnz, Np), dtype=torch.float32, device=E.device) if want_e else None
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        if given and M and (ptr(dB) is not None or ptr(dE) is not None):   # (else: no element to write)
            eng = _entry_for_parts(crow, col, val, ctx.shape, ctx.dev, ctx.fast, values_needed=False).eng
            Brm = _rowmajor(B.detach(), K, N, Np) if B is not None else None
            Erm = _rowmajor(E.detach(), nnz, N, Np)
            eng.spmm_edge_multi_backward_device_rm(ctx.op, Np, ptr(Brm), Brm.stride(0) if Brm is not None else Np, ptr(Erm), Erm.stride(0), g,
                                                   ptr(dB), Np, ptr(dE), Np, torch.cuda.current_stream(E.device).cuda_stream)
        elif given:
            for t in (dB, dE):
                if t is not None:
                    t.zero_()
        gB = (dB if Np == N else dB[:, :N]).to(B.dtype) if want_b else None
        gE = (dE if Np == N else dE[:, :N]).to(E.dtype) if want_e else None
        return (None, gB, gE) + none[3:]


def _check_edge_operands(A, B, E, op, name):
    """The misuse spmm_edge() refuses, for the 2-D operands of spmm_edge_multi() / spmm_edge_reduce()."""
    if op not in _EDGE_OPS:
        raise ValueError("op must be 'mul', 'add', 'add_relu' or 'copy'")
    _check_sparse(A, name)
    if (B is None) != (op == "copy"):
        raise ValueError(name + ": B=None goes with op='copy', and only with it")
    if not (isinstance(E, torch.Tensor) and E.is_cuda and (B is None or (isinstance(B, torch.Tensor) and B.is_cuda))):
        raise TypeError(name + " expects CUDA/HIP dense B and E")
    if E.dim() != 2 or (B is not None and (B.dim() != 2 or B.shape[1] != E.shape[1])):
        raise ValueError(name + ": B is (K, N), E (nnz, N)")
    if E.shape[0] != A.values().numel() or (B is not None and B.shape[0] != A.shape[1]) or E.shape[1] == 0:
        raise ValueError("shape mismatch")


def _edge_multi(A, B, E, op, want, place, width, fast, want_arg):
    """-> (out or None, {raw name: (M, N) tensor}, argmax, argmin) of the edge-feature multi-aggregation, through autograd when a
    gradient can be asked for (the args are then always computed)."""
    N = E.shape[1]
    code = _EDGE_OPS[op]
    if torch.is_grad_enabled() and ((B is not None and B.requires_grad) or E.requires_grad):
        out, *rest = _SpmmEdgeMultiFunction.apply(A, B, E, code, want, place, width, bool(fast))
        return out, {name: t for name, t in zip(_MULTI_RAW, rest[:4]) if t is not None}, rest[4], rest[5]
    out, raw, amax, amin = _multi_raw(A, B, want, place, width, bool(fast), want_arg, E, code)
    cut = lambda t: t if t is None or t.shape[1] == N else t[:, :N]
    return out, {name: cut(t) for name, t in raw.items()}, cut(amax), cut(amin)


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
    out, raw, _, _ = _edge_multi(A, B, E, op, want, place, width, fast, False)
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
    _, raw, amax, amin = _edge_multi(A, B, E, op, (name,), {}, E.shape[1], fast, bool(return_arg))
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
