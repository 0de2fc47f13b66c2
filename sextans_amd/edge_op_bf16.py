"""edge_op.edge_op() with its (nnz, N) tensors in bf16: Z is returned in bf16, E and the upstream gradient are bf16 and are read where they
lie (sextans_edge_op_device_rm_bf16 / sextans_edge_op_backward_device_rm_bf16) -- what autocast hands over and what the next Linear
wants, without fp32 copies of the largest tensors of a model.
Public: edge_op_bf16().  A function of its own next to edge_op(), whose parameter list and result dtype stay what they are; the checks,
the autograd function and the cached engines are edge_op's (torch_op.cache_info() / clear_cache() cover it)."""
from .edge_op import _edge_op

__all__ = ["edge_op_bf16"]


def edge_op_bf16(A, x_dst=None, x_src=None, E=None, op="add", fast=False):
    """edge_op(A, x_dst, x_src, E, op) with the (nnz, N) tensors in bf16: operands, ops, shapes and misuse are edge_op()'s, except that E
    must be None or a bf16 tensor -- with N % 8 == 0 one the kernel can read where it lies (row-major, 16-byte aligned base and rows);
    ValueError otherwise; an N that is not a multiple of 8 takes a zero-padded bf16 copy -- and that the result is bf16.  The
    arithmetic does not change: a bf16 value is widened exactly, every operation and sum is fp32, Z is the fp32 result rounded once to
    nearest even -- the bits of edge_op(A, x_dst, x_src, E.float(), op).to(torch.bfloat16) from ONE kernel pass, with no fp32
    (nnz, N) tensor anywhere.  Differentiable in x_dst, x_src and E: the upstream gradient, which autograd hands over in bf16, is read as
    it lies and IS E's gradient; the endpoint gradients are the bits of edge_op()'s on the widened upstream gradient, returned in the
    operands' dtype.  x_dst and x_src stay fp32 (another dtype is widened by a copy: they are (M, N))."""
    return _edge_op(A, x_dst, x_src, E, op, fast, True)
