"""gated.spmm_gated() with its (nnz, N) tensors in bf16: z is returned in bf16, E and the upstream gradient of z are bf16 and are read where
they lie, E's gradient is written in bf16 (sextans_spmm_gated_device_rm_bf16 / sextans_spmm_gated_backward_device_rm_bf16) -- what
autocast hands over and what the next Linear wants, without fp32 copies of the largest tensors of a GatedGCN layer.
Public: spmm_gated_bf16().  A function of its own next to spmm_gated(), whose parameter list and result dtypes stay what they are; the
checks, the autograd function and the cached engines are spmm_gated's (torch_op.cache_info() / clear_cache() cover it)."""
from .gated import _spmm_gated

__all__ = ["spmm_gated_bf16"]


def spmm_gated_bf16(A, x_dst, x_src, V, E=None, normalize=False, eps=1e-6, return_edge=False, fast=False):
    """spmm_gated(A, x_dst, x_src, V, E, normalize, eps, return_edge) with the (nnz, N) tensors in bf16: operands, modes, shapes and misuse
    are spmm_gated()'s, except that E must be None or a bf16 tensor (ValueError otherwise) -- read where it lies when it is row-major and
    16-byte aligned with N % 8 == 0, through a zero-padded bf16 copy otherwise -- and that z is returned in bf16.  The arithmetic does not
    change: a bf16 value is widened exactly, every operation and sum is fp32, the gates come from the unrounded fp32 z and only the stored
    z is rounded, once, to nearest even -- C (fp32) has the bits of spmm_gated(A, x_dst, x_src, V, E.float(), ...) and z is its z
    .to(torch.bfloat16), from ONE kernel pass with no fp32 (nnz, N) tensor anywhere.  Differentiable in x_dst, x_src, V and E through
    both outputs: the upstream gradient of z, which autograd hands over in bf16, is read as it lies when it qualifies; E's gradient is
    written in bf16 by the kernel (the fp32 one rounded once), the node gradients are the bits of spmm_gated()'s on the widened upstream
    gradient, returned in the operands' dtype.  x_dst, x_src and V stay fp32 (another dtype is widened by a copy: they are node-sized)."""
    return _spmm_gated(A, x_dst, x_src, V, E, normalize, eps, return_edge, fast, True)
