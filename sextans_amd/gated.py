"""Gated aggregation for torch: the message passing of ResGatedGraphConv (PyG) and GatedGCN (Bresson & Laurent; the MPNN of GraphGPS) as
one fused pass over a sparse_csr pattern per direction.  Public: spmm_gated().  The other ops of the torch front end live in
sextans_amd.torch_op; this one shares their cached engines (torch_op.cache_info() / clear_cache() cover it) and the frame of the tiled
families in _op_aggregate.py."""
import math

import torch
from torch.autograd.function import once_differentiable

from . import api
from ._op_aggregate import _any_elements, _edge_bf16, _rowmajor_ld, _tiled_entry
from ._op_cache import (_check_dense, _check_sparse, _cut, _cut_grad, _f32, _index_tensors, _keep_pattern, _kept_pattern_entry,
                        _ptr_nonempty)

__all__ = ["spmm_gated"]


def _gated_in(x_dst, x_src, V, E, M, K, N, Np, bf16=False):
    """-> (the GatedIn of a call, the tensors it points to -- to be kept alive over the call).  bf16: E is handed over in bf16 (the struct
    serves both entry points), as it lies when it qualifies."""
    nnz = E.shape[0] if E is not None else 0
    keep = [_rowmajor_ld(t, rows, N, Np) for t, rows in ((x_dst, M), (x_src, K), (V, K))]
    keep.append(_rowmajor_ld(E, nnz, N, Np, torch.bfloat16 if bf16 else torch.float32))
    gin = api.GatedIn()
    for name, (t, ld) in zip(("xdst", "xsrc", "v", "e"), keep):
        setattr(gin, "d_" + name, _ptr_nonempty(t))
        setattr(gin, "ld_" + name, ld)
    return gin, keep


def _gated_forward(A, x_dst, x_src, V, E, mode, eps, want_den, want_z, fast, bf16=False):
    """(C, den, z) of the engine's gated aggregation: C and den (M, Np), z (nnz, Np) with N padded up to a multiple of 8 (zero columns of
    the operands); den and z None unless asked for.  bf16: E (a bf16 tensor, or None) and z in bf16, through
    sextans_spmm_gated_device_rm_bf16; C and den fp32 either way."""
    N = x_dst.shape[1]
    M, K, Np, ent, stream, val = _tiled_entry(A, N, fast)
    gin, keep = _gated_in(x_dst, x_src, V, E, M, K, N, Np, bf16)
    C = _f32(A.device, M, Np)
    den = _f32(A.device, M, Np) if want_den else None
    z = torch.empty((val.numel(), Np), dtype=torch.bfloat16 if bf16 else torch.float32, device=A.device) if want_z else None
    if _any_elements(C, z):
        call = ent.eng.spmm_gated_device_rm_bf16 if bf16 else ent.eng.spmm_gated_device_rm
        call(mode, eps, Np, gin, _ptr_nonempty(C), Np, _ptr_nonempty(den), Np, _ptr_nonempty(z), Np, stream)
    del keep
    return C, den, z


class _SpmmGatedFunction(torch.autograd.Function):
    """spmm_gated(): ONE forward call (sextans_spmm_gated_device_rm) that keeps C and the gates' sums in normalize mode and nothing of size
    nnz x N beyond the z output that was asked for; ONE backward call (sextans_spmm_gated_backward_device_rm) for the gradients autograd
    wants -- a row pass over A for x_dst and E, a column pass over A^T for x_src and V -- with the gates recomputed.  z's upstream
    gradient is the call's Gz.  A's values never enter: no gradient for A, no value refresh.  Not twice differentiable.  bf16: the _bf16
    entry points -- E, z, z's upstream gradient and E's gradient in bf16, read and written where they lie (one dtype for all (nnz, N)
    tensors of a call); C, its upstream gradient and the node gradients fp32 as before."""

    @staticmethod
    def forward(ctx, A, x_dst, x_src, V, E, mode, eps, want_z, fast, bf16=False):
        N = x_dst.shape[1]
        norm = mode == api.GATE_NORM
        C, den, z = _gated_forward(A, x_dst, x_src, V, E, mode, eps, norm, want_z, fast, bf16)
        ctx.save_for_backward(*_index_tensors(A), A.values(), x_dst, x_src, V, E, *((C, den) if norm else ()))
        _keep_pattern(ctx, A, fast)
        ctx.mode, ctx.eps, ctx.bf16 = mode, eps, bf16
        ctx.set_materialize_grads(False)
        return _cut(C, N), _cut(z, N)

    @staticmethod
    @once_differentiable
    def backward(ctx, G, Gz):
        crow, col, val, x_dst, x_src, V, E, *fwd = ctx.saved_tensors
        C, den = fwd if fwd else (None, None)
        M, K = ctx.shape
        nnz, N = val.numel(), x_dst.shape[1]
        Np = api.round_up_n(N)
        want = dict(zip(("dxdst", "dxsrc", "dv", "de"), (ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.needs_input_grad[3],
                                                         E is not None and ctx.needs_input_grad[4])))
        none = (None,) * 10
        e_dtype = torch.bfloat16 if ctx.bf16 else torch.float32
        if not any(want.values()) or (G is None and Gz is None):
            return none
        rows = {"dxdst": M, "dxsrc": K, "dv": K, "de": nnz}
        bufs = {name: torch.empty((rows[name], Np), dtype=e_dtype if name == "de" else torch.float32, device=val.device)
                for name, w in want.items() if w}
        if _any_elements(*bufs.values()):
            ent, stream = _kept_pattern_entry(ctx, crow, col, val)
            if G is None:   # only z was used downstream
                Grm, ldg = torch.zeros((M, Np), dtype=torch.float32, device=val.device), Np
            else:
                Grm, ldg = _rowmajor_ld(G, M, N, Np)           # (a copy when G has zero strides, e.g. after .sum(), or N % 8 != 0)
            Gzrm, ldgz = _rowmajor_ld(Gz, nnz, N, Np, e_dtype)   # (bf16: read as it lies when it qualifies, a copy stays bf16)
            gin, keep = _gated_in(x_dst, x_src, V, E, M, K, N, Np, ctx.bf16)
            out = api.GatedGrad()
            for name, t in bufs.items():
                setattr(out, "d_" + name, _ptr_nonempty(t))
                setattr(out, "ld_" + name, Np)
            nwork = ent.eng.spmm_gated_workspace_floats(ctx.mode, Np)
            work = _f32(val.device, nwork) if nwork else None
            call = ent.eng.spmm_gated_backward_device_rm_bf16 if ctx.bf16 else ent.eng.spmm_gated_backward_device_rm
            call(ctx.mode, ctx.eps, Np, gin, _ptr_nonempty(C), Np, _ptr_nonempty(den), Np, _ptr_nonempty(Grm), ldg, _ptr_nonempty(Gzrm), ldgz,
                 out, _ptr_nonempty(work), stream)
            del keep
        return (None, _cut_grad(bufs.get("dxdst"), N, x_dst), _cut_grad(bufs.get("dxsrc"), N, x_src), _cut_grad(bufs.get("dv"), N, V),
                _cut_grad(bufs.get("de"), N, E) if E is not None else None) + none[5:]


def spmm_gated(A, x_dst, x_src, V, E=None, normalize=False, eps=1e-6, return_edge=False, fast=False):
    """Gated aggregation: every stored entry e = (r, c) of A gets a per-channel sigmoid gate from both of its endpoints and, optionally,
    its own features, and gates the message V[c]:
        z_e = x_dst[r] + x_src[c] (+ E[e])        g_e = sigmoid(z_e)
        C[r] = sum_e g_e * V[c]                               normalize=False: ResGatedGraphConv (PyG)
        C[r] = sum_e g_e * V[c] / (sum_e g_e + eps)           normalize=True:  GatedGCN (Bresson & Laurent), GraphGPS's MPNN
    A is an (M, K) sparse_csr matrix of which only the PATTERN is used (its values are not read, the cached engine is not refreshed and A
    gets no gradient); x_dst is (M, N), x_src and V are (K, N), E is (nnz, N) IN A'S CSR ENTRY ORDER (torch_op.from_edge_index() gives the
    permutation for an edge list).  Returns the dense fp32 (M, N) tensor C, or (C, z) with return_edge=True: z (nnz, N) are the
    pre-activations, GatedGCN's new edge features (before its BatchNorm, ReLU and residual).  A row without entries gives 0.
    One kernel pass per direction (sextans_spmm_gated_device_rm / _backward_device_rm): without E and z nothing of size nnz x N exists;
    the backward recomputes the gates instead of storing them; no atomics -- the same bits on every run.  Differentiable in x_dst, x_src,
    V and E through both outputs; only the gradients asked for are computed.  normalize=True needs a finite eps > 0.  An N that is not a
    multiple of 8, and operands the kernel cannot read where they lie, are copied with zero padding, as torch_op.spmm_edge() does; `fast`
    only selects the cached engine.  With return_edge=False a bf16 E (autocast) with N % 8 == 0 that is row-major and 16-byte aligned is read
    as it lies and its gradient written in bf16 by the kernel (sextans_spmm_gated_device_rm_bf16 / _backward_device_rm_bf16): the bits of
    the route through an fp32 copy of E, without an fp32 (nnz, N) tensor; C stays fp32.  The same op with z in bf16 too:
    sextans_amd.gated_bf16.spmm_gated_bf16()."""
    return _spmm_gated(A, x_dst, x_src, V, E, normalize, eps, return_edge, fast, False)


def _spmm_gated(A, x_dst, x_src, V, E, normalize, eps, return_edge, fast, bf16):
    """spmm_gated() (bf16 False: the bf16 entry points only where they return the fp32 route's bits and dtypes -- no z, a qualifying bf16
    E) and gated_bf16.spmm_gated_bf16() (True: all (nnz, N) tensors in bf16): the checks and the call, once"""
    _check_sparse(A, "spmm_gated")
    _check_dense("spmm_gated", "x_dst, x_src, V and E", x_dst, x_src, V, *(() if E is None else (E,)))
    M, K = A.shape
    if x_dst.dim() != 2 or x_src.dim() != 2 or V.dim() != 2 or (E is not None and E.dim() != 2):
        raise ValueError("spmm_gated: x_dst is (M, N), x_src and V (K, N), E (nnz, N)")
    N = x_dst.shape[1]
    if N == 0 or tuple(x_dst.shape) != (M, N) or tuple(x_src.shape) != (K, N) or tuple(V.shape) != (K, N) or \
            (E is not None and tuple(E.shape) != (A.values().numel(), N)):
        raise ValueError("shape mismatch")
    eps = float(eps)
    if normalize and not (eps > 0.0 and math.isfinite(eps)):
        raise ValueError("spmm_gated: normalize=True needs a finite eps > 0")
    mode = api.GATE_NORM if normalize else api.GATE_SUM
    if bf16:
        if E is not None and E.dtype != torch.bfloat16:
            raise ValueError("spmm_gated_bf16 takes E=None or a bf16 E (one dtype for all (nnz, N) tensors of a call)")
    else:
        bf16 = not return_edge and _edge_bf16(E, N)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x_dst, x_src, V, E)):
        C, z = _SpmmGatedFunction.apply(A, x_dst, x_src, V, E, mode, eps, bool(return_edge), bool(fast), bf16)
    else:
        C, _, z = (_cut(t, N) for t in _gated_forward(A, x_dst, x_src, V, E, mode, eps, False, bool(return_edge), bool(fast), bf16))
    return (C, z) if return_edge else C
