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

The gated aggregation of ResGatedGraphConv / GatedGCN (a per-channel sigmoid gate per entry from both endpoints and the entry's features)
lives in a module of its own, on the same cached engines: sextans_amd.gated.spmm_gated(A, x_dst, x_src, V, E=None, normalize=False, ...)
(with the (nnz, N) tensors in bf16: sextans_amd.gated_bf16.spmm_gated_bf16).
So does the softmax aggregation of edge-feature messages (GENConv / DeeperGCN with edge features: relu(x_j + e_ij) + eps under a softmax
with a learnable temperature): sextans_amd.edge_softagg.spmm_edge_softagg(A, B, E, op="mul", t=1.0, eps=0.0, return_lse=False).
And Point Transformer's channel-wise attention from per-channel scores: sextans_amd.vector_attention.vector_attention(A, S, V=None, D=None).
The opposite direction, node to edge -- the (nnz, N) tensors those ops read, from both endpoints of every entry (u_add_v, u_sub_v, u_mul_v,
copy_u, copy_v, each optionally + e), with a backward without atomics: sextans_amd.edge_op.edge_op(A, x_dst=None, x_src=None, E=None, op="add")
(with the (nnz, N) tensors in bf16: sextans_amd.edge_op_bf16.edge_op_bf16).
And the (nnz, H) scores score_attention() reads, the per-head dot product of both endpoints (u_dot_v), all heads in one launch dealt by
non-zeros: sextans_amd.edge_dot.edge_dot(A, x_dst, x_src).

Edge features INSIDE the fused attention (TransformerConv(edge_dim=...), UniMP, relative-position encodings), one kernel pass per direction:

    O = sparse_attention_edge(A, Q, K, V, edge_key=None, edge_value=None, scale=None, bias=False, dropout=0.0, seed=None, step=None)
                                                   softmax(scale * (<Q[r], K[c] + edge_key[e]> [+ A_e])) (V[c] + edge_value[e]) per head;
                                                   the edge tensors are (nnz, H, d) in A's entry order; edge_key is edge_value: one gradient

S and P are sparse_csr tensors that carry A's own index tensors, so the three ops and spmm() meet in one cache entry and hand each
other's values to the engine as value refreshes; all are differentiable, their backward passes run on the engine too.
"""
# This module is the public import point; the code lives in four private siblings (no cycles: each imports only those above it):
#   _op_cache      the engine cache (one entry per pattern) and the operand helpers every op uses
#   _op_product    spmm, sddmm, row_softmax
#   _op_attention  the fused attention families (one frame, five Functions), dropout, the composition
#   _op_aggregate  the tiled aggregation families (one frame): reduce, softagg, multi, edge, edge_multi; from_edge_index
from ._op_cache import _MAX_ENGINES, _cache, _carry, _grad_values, _index_tensors, _rowmajor, cache_info, clear_cache, refresh  # noqa: F401
from ._op_product import row_softmax, sddmm, spmm  # noqa: F401
from ._op_attention import (_check_dropout, _heads_operand, _scalars_operand, dropout_mask, entry_rows, gat_attention,  # noqa: F401
                            gat_attention_dropout, gatv2_attention, gatv2_attention_dropout, score_attention, sparse_attention,
                            sparse_attention_dropout, sparse_attention_edge)
from ._op_aggregate import (_MULTI_NEEDS, from_edge_index, spmm_edge, spmm_edge_multi, spmm_edge_reduce, spmm_multi, spmm_reduce,  # noqa: F401
                            spmm_softagg)
