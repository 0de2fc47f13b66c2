"""The product ops of the torch front end (private; sextans_amd.torch_op is the public import point): spmm, sddmm, row_softmax."""
import torch
from torch.autograd.function import once_differentiable

from . import api
from ._op_cache import (_carry, _check_sparse, _cut_grad, _engine_for, _engine_for_parts, _entry_for_parts, _grad_values, _index_tensors,
                        _ptr, _qualifies, _rowmajor, _vals32)


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
            gB = _cut_grad(out, N, B)
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
            ent.eng.sddmm_device_rm(Np, alpha, Xr.data_ptr(), Xr.stride(0), Yr.data_ptr(), Yr.stride(0), beta, _ptr(vin), out.data_ptr(),
                                    torch.cuda.current_stream(A.device).cuda_stream)
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
                gX = _cut_grad(out, N, X)
            if ctx.needs_input_grad[2]:
                Xr = _rowmajor(X.detach(), M, N, Np)
                out = torch.zeros((K, Np), dtype=torch.float32, device=g.device)
                eng.spmm_t_device_rm(Np, ctx.alpha, Xr.data_ptr(), Xr.stride(0), 0.0, out.data_ptr(), Np, out.data_ptr(), Np, stream)
                gY = _cut_grad(out, N, Y)
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
