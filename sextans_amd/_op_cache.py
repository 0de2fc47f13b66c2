"""The torch front end's engine cache and operand helpers (private; sextans_amd.torch_op is the public import point): one cached
engine per sparsity pattern, and the few functions every op uses to hand tensors to the engine where they lie."""
import collections
import weakref

import torch

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


# --- the pattern passes' way to the engine: A's values go to the kernels as a pointer, never through the engine (no value refresh) ----
def _pattern_entry(crow, col, val, shape, dev, fast):
    """-> (the cached entry of the pattern, its values left as they are; the current stream)"""
    return _entry_for_parts(crow, col, val, shape, dev, fast, values_needed=False), torch.cuda.current_stream(val.device).cuda_stream


def _pattern_entry_of(A, fast):
    """_pattern_entry() of a sparse_csr tensor -> (entry, stream, crow, col, val).  A Function saves the last three for its backward
    and calls _keep_pattern(); the backward then comes back to the entry through _kept_pattern_entry()."""
    crow, col = _index_tensors(A)
    val = A.values()
    return _pattern_entry(crow, col, val, tuple(A.shape), A.device.index or 0, fast) + (crow, col, val)


def _keep_pattern(ctx, A, fast):
    ctx.shape, ctx.dev, ctx.fast = tuple(A.shape), A.device.index or 0, fast


def _kept_pattern_entry(ctx, crow, col, val):
    return _pattern_entry(crow, col, val, ctx.shape, ctx.dev, ctx.fast)


# --- operands ------------------------------------------------------------------------------------------------------------------------
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


def _check_dense(name, what, *tensors):
    """the operands named in `what` are CUDA/HIP tensors"""
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors):
        raise TypeError("%s expects CUDA/HIP dense %s" % (name, what))


def _ptr(t):
    """an optional operand's address: None -> NULL"""
    return t.data_ptr() if t is not None else None


def _ptr_nonempty(t):
    """an optional operand's address: None, or a tensor without elements (whose address may be anything) -> NULL"""
    return t.data_ptr() if t is not None and t.numel() else None


def _f32(device, *shape):
    return torch.empty(shape, dtype=torch.float32, device=device)


def _cut(t, n):
    """a padded buffer's last dimension cut back to n (t itself when nothing was padded); None stays None"""
    return t if t is None or t.shape[-1] == n else t[..., :n]


def _cut_grad(buf, n, like, wanted=True):
    """a padded gradient buffer as autograd wants it: cut back to n, in the operand's dtype -- None where no gradient is wanted or made"""
    return _cut(buf, n).to(like.dtype) if wanted and buf is not None else None


def _pattern_grad(crow, col, val, dvals, shape):
    """the gradient of A from that of its values (None: none wanted): a sparse_csr tensor on A's index tensors, in A's value dtype"""
    return torch.sparse_csr_tensor(crow, col, dvals.to(val.dtype), size=shape) if dvals is not None else None


def _row_degrees(A, dtype):
    """(M, 1): every row's stored-entry count clamped to >= 1, what "mean" divides by"""
    crow = _index_tensors(A)[0]
    return (crow[1:] - crow[:-1]).clamp(min=1).to(dtype)[:, None]
