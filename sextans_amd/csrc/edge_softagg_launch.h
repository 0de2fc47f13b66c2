// edge_softagg_launch.h -- what the objects of the edge-feature softmax aggregation share: the launchers and the bodies of the two entry
// points, for one element type ET of the (nnz, N) tensors E and dE (spmm_edge_softagg_kernels.h).  engine_edge_softagg.hip instantiates
// ET = float (sextans_spmm_edge_softagg_device_rm, sextans_spmm_edge_softagg_backward_device_rm, and the workspace size, which serves
// both element types), engine_edge_softagg_bf16.hip and engine_edge_softagg_bf16_backward.hip ET = uint16_t (the _bf16 entry points):
// the kernels of one element type and direction are compiled in one object each, the checks, their order and the passes are one text.
// The row pass runs when dE or dt is asked for.  It keeps the dt sum whether or not dt is asked for, as engine_softagg.hip's does and for
// its reason, and its dE store is PREDICATED on the pointer, not a compile-time switch: a variant without the store would add 4 ops x
// 4 widths x 2 kernels for the call that wants dt alone, and what the predicate saves there -- the stores, not the E stream, which the
// messages need anyway -- a wavefront-uniform branch saves as well.
#pragma once
#include "pattern_launch.h"
#include "spmm_edge_softagg_kernels.h"

namespace sxe {
namespace {

// e: the engine whose CSR arrays and softmax tables the pass walks (the column pass: the companion).  N is cut into tiles of the smallest
// of 8 / 16 / 32 / 64 floats that holds min(N, kMaxTile); the last tile may be partial; the tiles sit in the grid in every pass (the row
// pass too: an (entry, tile) of dE belongs to one slot).  THE TILE IS CAPPED AT 64 FLOATS: spmm_softagg's row pass takes all 256 VGPRs at
// 128, and these passes carry an E row per entry in flight on top of it.
// Entries in flight per slot (U), all UNTUNED -- no other value has been timed: 4 in the forward (it MUST equal engine_softagg.hip's 4:
// with E[e, :] = val[e] under MUL the forward then returns spmm_softagg's bits, which tests/test_spmm_edge_softagg_gpu.py pins) and in the
// row pass (an entry costs a gathered B row and its E row), 2 in the column pass (three gathered rows -- C, lse, G -- and the E row).
// No kernel uses scratch or spills at these values (profiles/spmm_edge_softagg_kernel_resources.txt).
// The slot geometry does NOT depend on ET: the order of every sum, and with it every fp32 bit, is the same for both element types.
constexpr int kMaxTile = 64;

template <int PASS, int OP, class ET>
void launch_pass(const sextans_engine *e, const sx::EdgeSoftaggArgsT<ET> &a, const int *perm, hipStream_t s) {
    for_width(a.N < kMaxTile ? a.N : kMaxTile, [&](auto w) {
        using W = decltype(w);
        constexpr int U = PASS == sx::kAttnBackwardCols ? 2 : 4;
        if constexpr (4 * W::T * W::P <= kMaxTile) launch_pattern<sx::EdgeSoftaggPass<PASS, OP, W::T, W::P, U, ET>>(e, tiled<W>(a), perm, false, s);
    });
}

template <int PASS, class ET>
void launch_op(int op, const sextans_engine *e, const sx::EdgeSoftaggArgsT<ET> &a, const int *perm, hipStream_t s) {
    if (op == SEXTANS_EDGE_MUL) launch_pass<PASS, sx::kEdgeMul>(e, a, perm, s);
    else if (op == SEXTANS_EDGE_ADD) launch_pass<PASS, sx::kEdgeAdd>(e, a, perm, s);
    else if (op == SEXTANS_EDGE_ADD_RELU) launch_pass<PASS, sx::kEdgeAddRelu>(e, a, perm, s);
    else if constexpr (PASS != sx::kAttnBackwardCols) launch_pass<PASS, sx::kEdgeCopy>(e, a, perm, s);   // (COPY has no dB)
}

inline bool bad_op(int op) { return op < SEXTANS_EDGE_MUL || op > SEXTANS_EDGE_COPY; }
// B is optional with COPY only
inline bool bad_ldb(int op, const float *d_B, int64_t ldb, int N) { return op == SEXTANS_EDGE_COPY ? bad_ld_of(d_B, ldb, N) : bad_ld(ldb, N); }

// The forward entry point; name: what sextans_last_kernel reads afterwards.  Leading dimensions are counted in elements of their tensor
// and are multiples of 4 for either element type (a bf16 piece is 8 bytes).
template <class ET>
int edge_softagg_forward(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const ET *d_E, int64_t lde, const float *d_t,
                         float *d_C, int64_t ldc, float *d_lse, int64_t ldlse, void *stream, const char *name) {
    if (!h || bad_op(op) || bad_n(N) || too_many_tiles(N, kMaxTile)) return SEXTANS_ERR_INVALID;   // nothing here needs a device
    if (bad_ldb(op, d_B, ldb, N) || bad_ld(lde, N) || bad_ld(ldc, N) || bad_ld_of(d_lse, ldlse, N)) return SEXTANS_ERR_INVALID;
    if (misaligned(d_B, d_E, d_t, d_C, d_lse)) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    if (int rc = call.open((!d_B && op != SEXTANS_EDGE_COPY) || !d_E || !d_C, stream)) return rc;
    if (call.degenerate()) {   // every row is empty
        attention_fill(d_C, h->M, N, ldc, 0.0f, call.s);
        attention_fill(d_lse, h->M, N, ldlse, -INFINITY, call.s);
        return call.done();
    }
    if (int rc = call.tables(false)) return rc;
    sx::EdgeSoftaggArgsT<ET> a{};
    a.B = d_B; a.E = d_E; a.t = d_t; a.out = d_C; a.out_lse = d_lse;
    a.ldb = ldb; a.lde = lde; a.ldc = ldc; a.ldlse = ldlse; a.N = N;
    call.rows([&](const sextans_engine *e, const int *perm) { launch_op<sx::kAttnForward>(op, e, a, perm, call.s); });
    return call.close(name);
}

template <class ET>
int edge_softagg_backward(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const ET *d_E, int64_t lde, const float *d_t,
                          const float *d_C, int64_t ldc, const float *d_lse, int64_t ldlse, const float *d_G, int64_t ldg, float *d_dB,
                          int64_t lddb, ET *d_dE, int64_t ldde, float *d_dt, float *d_work, void *stream, const char *name) {
    if (!h || bad_op(op) || bad_n(N) || too_many_tiles(N, kMaxTile)) return SEXTANS_ERR_INVALID;
    if (bad_ldb(op, d_B, ldb, N) || bad_ld(lde, N) || bad_ld(ldc, N) || bad_ld(ldlse, N) || bad_ld(ldg, N) || bad_ld_of(d_dB, lddb, N) ||
        bad_ld_of(d_dE, ldde, N))
        return SEXTANS_ERR_INVALID;
    if (misaligned(d_B, d_E, d_t, d_C, d_lse, d_G, d_dB, d_dE, d_dt, d_work)) return SEXTANS_ERR_INVALID;
    if (!d_dB && !d_dE && !d_dt) return SEXTANS_ERR_INVALID;   // nothing to compute
    if (d_dt && !d_work) return SEXTANS_ERR_INVALID;
    if (d_dB && op == SEXTANS_EDGE_COPY) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    if (int rc = call.open((!d_B && op != SEXTANS_EDGE_COPY) || !d_E || !d_C || !d_lse || !d_G, stream)) return rc;
    float *d_rows = d_dt ? d_work : nullptr;   // the workspace is written only for dt
    float *d_part = d_rows ? d_rows + (int64_t)h->M * N : nullptr;
    if (call.degenerate()) {   // (dE has no element)
        attention_fill(d_dB, h->K, N, lddb, 0.0f, call.s);
        attention_fill(d_rows, h->M, N, N, 0.0f, call.s);   // dt_rows and the chunk sums: what the passes would have left
        attention_fill(d_part, chunks_of(h->M), N, N, 0.0f, call.s);
        attention_fill(d_dt, 1, N, N, 0.0f, call.s);
        return call.done();
    }
    if (int rc = call.tables(d_dB != nullptr)) return rc;
    sx::EdgeSoftaggArgsT<ET> a{};
    a.B = d_B; a.E = d_E; a.t = d_t; a.C = d_C; a.lse = d_lse; a.G = d_G;
    a.dB = d_dB; a.dE = d_dE; a.dt_rows = d_rows;
    a.ldb = ldb; a.lde = lde; a.ldc = ldc; a.ldlse = ldlse; a.ldg = ldg; a.lddb = lddb; a.ldde = ldde; a.N = N;
    if (d_dB) call.cols([&](const sextans_engine *e, const int *perm) { launch_op<sx::kAttnBackwardCols>(op, e, a, perm, call.s); });
    if (d_dE || d_dt) call.rows([&](const sextans_engine *e, const int *perm) { launch_op<sx::kAttnBackwardRows>(op, e, a, perm, call.s); });
    if (d_dt) column_sum_two_level(d_rows, h->M, N, d_part, d_dt, call.s);
    return call.close(name);
}

}  // namespace
}  // namespace sxe
