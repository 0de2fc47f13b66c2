"""The public surface of sextans_amd.torch_op, pinned: the 23 public functions by name and signature, their place in the module docstring,
the private names tests and tools reach through the module, and the identity of the cache dict.  torch_op is the one import point of a
front end that lives in private sibling modules; importing it needs no GPU."""
import inspect

SIGNATURES = {
    "clear_cache": "()",
    "cache_info": "()",
    "refresh": "(A, fast=False)",
    "spmm": "(A, B, alpha=1.0, beta=0.0, C=None, out=None, fast=False, transpose_a=False, out_dtype=None)",
    "sddmm": "(A, X, Y, alpha=1.0, beta=0.0, fast=False)",
    "row_softmax": "(S, scale=1.0, fast=False)",
    "dropout_mask": "(A, heads, p, seed, step=None)",
    "sparse_attention": "(A, Q, K, V, scale=None, bias=False, fast=False, fused=False)",
    "sparse_attention_dropout": "(A, Q, K, V, dropout, seed=None, step=None, scale=None, bias=False, fast=False, fused=False)",
    "sparse_attention_edge": "(A, Q, K, V, edge_key=None, edge_value=None, scale=None, bias=False, dropout=0.0, seed=None, step=None, fast=False)",
    "gat_attention": "(A, a_dst, a_src, V, negative_slope=0.2, bias=False, fast=False)",
    "gat_attention_dropout": "(A, a_dst, a_src, V, dropout, seed=None, step=None, negative_slope=0.2, bias=False, fast=False)",
    "entry_rows": "(A)",
    "score_attention": "(A, S, V, normalize='softmax', dropout=0.0, seed=None, step=None, return_weights=False, fast=False)",
    "gatv2_attention": "(A, x_dst, x_src, att, negative_slope=0.2, bias=False, fast=False)",
    "gatv2_attention_dropout": "(A, x_dst, x_src, att, dropout, seed=None, step=None, negative_slope=0.2, bias=False, fast=False)",
    "spmm_reduce": "(A, B, reduce='amax', return_arg=False, fast=False)",
    "spmm_softagg": "(A, B, t=1.0, return_lse=False, fast=False)",
    "spmm_multi": "(A, B, aggr=('mean', 'max', 'min', 'std'), eps=1e-05, fast=False)",
    "spmm_edge": "(A, B, E, op='mul', reduce='sum', fast=False)",
    "spmm_edge_multi": "(A, B, E, op='mul', aggr=('mean', 'max', 'min', 'std'), eps=1e-05, fast=False)",
    "spmm_edge_reduce": "(A, B, E, op='mul', reduce='amax', return_arg=False, fast=False)",
    "from_edge_index": "(edge_index, num_dst, num_src, values=None)",
}
PRIVATE = ("_cache", "_MAX_ENGINES", "_MULTI_NEEDS", "_check_dropout", "_rowmajor", "_index_tensors", "_grad_values", "_carry",
           "_heads_operand", "_scalars_operand")


def test_the_public_functions_and_their_signatures():
    from sextans_amd import torch_op
    assert len(SIGNATURES) == 23
    for name, sig in SIGNATURES.items():
        fn = getattr(torch_op, name)
        assert inspect.isfunction(fn), name
        assert str(inspect.signature(fn)) == sig, name
        assert fn.__doc__, name
    public = {name for name, fn in vars(torch_op).items() if inspect.isfunction(fn) and not name.startswith("_")}
    assert public == set(SIGNATURES)


def test_every_public_function_is_in_the_module_docstring():
    from sextans_amd import torch_op
    for name in SIGNATURES:
        assert name in torch_op.__doc__, name


def test_private_names_resolve_and_the_cache_is_the_cache_modules_own():
    from sextans_amd import _op_cache, torch_op
    for name in PRIVATE:
        assert hasattr(torch_op, name), name
    assert torch_op._cache is _op_cache._cache
    assert torch_op.clear_cache is _op_cache.clear_cache and torch_op.clear_cache.__globals__["_cache"] is torch_op._cache
