// edge_multi_launch.h -- the launcher of the edge-feature multi-aggregation (spmm_edge_multi_kernels.h), shared by engine_edge_multi.hip
// (the entry points) and engine_edge_multi_mul.hip / _add.hip / _add_relu.hip / _copy.hip and included by nothing else.  The family has
// 3 passes x 4 ops x 3 groups x 4 widths x 2 kernels; one source per op instantiates its share, so that the objects compile side by side
// and none takes longer than engine_multi.hip's.
#pragma once
#include "pattern_launch.h"
#include "spmm_edge_multi_kernels.h"

namespace sxe {

// THIS FAMILY'S TILE IS CAPPED AT 64 FLOATS, as engine_multi.hip's and for the same reason (6 floats of state per column in the forward
// and a second copy in the merge); this forward keeps an E row per entry in flight on top of the gathered B row.
// Entries in flight per slot (U): 2 in the forward and the row pass (an entry costs up to two loads of a tile's pieces), 1 in the
// column pass (up to six gathered rows and the E row per entry).  Untuned starting values.
constexpr int kEdgeMultiMaxTile = 64;

// One pass of one op; e: the engine whose CSR arrays and softmax tables the pass walks (the column pass: the companion).  The tiles sit
// in the grid in every pass (the row pass too: an (entry, tile) belongs to one slot).  Defined one per source.
void launch_edge_multi_mul(int pass, int groups, const sextans_engine *e, const sx::EdgeMultiArgs &a, const int *perm, hipStream_t s);
void launch_edge_multi_add(int pass, int groups, const sextans_engine *e, const sx::EdgeMultiArgs &a, const int *perm, hipStream_t s);
void launch_edge_multi_add_relu(int pass, int groups, const sextans_engine *e, const sx::EdgeMultiArgs &a, const int *perm, hipStream_t s);
void launch_edge_multi_copy(int pass, int groups, const sextans_engine *e, const sx::EdgeMultiArgs &a, const int *perm, hipStream_t s);

template <int PASS, int OP, int GROUPS>
void edge_multi_groups(const sextans_engine *e, const sx::EdgeMultiArgs &a, const int *perm, hipStream_t s) {
    for_width(a.N < kEdgeMultiMaxTile ? a.N : kEdgeMultiMaxTile, [&](auto w) {
        using W = decltype(w);
        constexpr int U = PASS == sx::kAttnBackwardCols ? 1 : 2;
        if constexpr (4 * W::T * W::P <= kEdgeMultiMaxTile)
            launch_pattern<sx::EdgeMultiPass<PASS, OP, GROUPS, W::T, W::P, U>>(e, tiled<W>(a), perm, false, s);
    });
}

template <int PASS, int OP>
void edge_multi_pass(int groups, const sextans_engine *e, const sx::EdgeMultiArgs &a, const int *perm, hipStream_t s) {
    if (groups == sx::kMultiMoments) edge_multi_groups<PASS, OP, sx::kMultiMoments>(e, a, perm, s);
    else if (groups == sx::kMultiExtrema) edge_multi_groups<PASS, OP, sx::kMultiExtrema>(e, a, perm, s);
    else edge_multi_groups<PASS, OP, sx::kMultiMoments | sx::kMultiExtrema>(e, a, perm, s);
}

// what a per-op source's function is
template <int OP>
void edge_multi_op(int pass, int groups, const sextans_engine *e, const sx::EdgeMultiArgs &a, const int *perm, hipStream_t s) {
    if (pass == sx::kAttnForward) edge_multi_pass<sx::kAttnForward, OP>(groups, e, a, perm, s);
    else if (pass == sx::kAttnBackwardRows) edge_multi_pass<sx::kAttnBackwardRows, OP>(groups, e, a, perm, s);
    else if constexpr (OP != sx::kEdgeCopy) edge_multi_pass<sx::kAttnBackwardCols, OP>(groups, e, a, perm, s);   // (COPY has no dB)
}

}  // namespace sxe
