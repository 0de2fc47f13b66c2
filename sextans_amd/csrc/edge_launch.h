// edge_launch.h -- what the two objects of the edge-feature SpMM share: the launchers and the bodies of the two entry points, for one
// element type ET of the (nnz, N) tensors E and dE (spmm_edge_kernels.h).  engine_edge.hip instantiates ET = float
// (sextans_spmm_edge_device_rm, sextans_spmm_edge_backward_device_rm), engine_edge_bf16.hip ET = uint16_t (the _bf16 entry points): the
// kernels of one element type are compiled in one object each, the checks, their order and the passes are one text.
#pragma once
#include "pattern_launch.h"
#include "spmm_edge_kernels.h"

namespace sxe {
namespace {

// e: the engine whose CSR arrays and softmax tables the pass walks (the column pass: the companion).  N is cut into tiles of the smallest
// of 8 / 16 / 32 / 64 / 128 floats that holds min(N, 128); the last tile may be partial; the tiles sit in the grid in every pass (the row
// pass too: an (entry, tile) belongs to one slot).  Entries in flight per slot (U): the reduce forward's 4 (2 at width 128) -- an entry
// costs up to two loads of a tile's pieces; untuned.
template <int PASS, int OP, class ET>
void launch_pass(const sextans_engine *e, const sx::EdgeArgsT<ET> &a, const int *perm, hipStream_t s) {
    for_width(a.N, [&](auto w) {
        using W = decltype(w);
        launch_pattern<sx::EdgePass<PASS, OP, W::T, W::P, W::k128 ? 2 : 4, ET>>(e, tiled<W>(a), perm, false, s);
    });
}

template <int PASS, class ET>
void launch_op(int op, const sextans_engine *e, const sx::EdgeArgsT<ET> &a, const int *perm, hipStream_t s) {
    if (op == SEXTANS_EDGE_MUL) launch_pass<PASS, sx::kEdgeMul>(e, a, perm, s);
    else if (op == SEXTANS_EDGE_ADD) launch_pass<PASS, sx::kEdgeAdd>(e, a, perm, s);
    else if (op == SEXTANS_EDGE_ADD_RELU) launch_pass<PASS, sx::kEdgeAddRelu>(e, a, perm, s);
    else if constexpr (PASS != sx::kAttnBackwardCols) launch_pass<PASS, sx::kEdgeCopy>(e, a, perm, s);   // (COPY has no dB)
}

inline bool bad_op(int op) { return op < SEXTANS_EDGE_MUL || op > SEXTANS_EDGE_COPY; }

// The forward entry point; name: what sextans_last_kernel reads afterwards.  Leading dimensions are counted in elements of their tensor
// and are multiples of 4 for either element type (a bf16 piece is 8 bytes).
template <class ET>
int spmm_edge_forward(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const ET *d_E, int64_t lde, float *d_C, int64_t ldc,
                      void *stream, const char *name) {
    if (!h || bad_op(op) || bad_n(N)) return SEXTANS_ERR_INVALID;   // nothing here needs a device
    if (bad_ld(ldb, N) || bad_ld(lde, N) || bad_ld(ldc, N)) return SEXTANS_ERR_INVALID;
    if (misaligned(d_B, d_E, d_C)) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    if (int rc = call.open((!d_B && op != SEXTANS_EDGE_COPY) || !d_E || !d_C, stream)) return rc;
    if (call.degenerate()) {   // every row is empty
        attention_fill(d_C, h->M, N, ldc, 0.0f, call.s);
        return call.done();
    }
    if (int rc = call.tables(false)) return rc;
    sx::EdgeArgsT<ET> a{};
    a.B = d_B; a.E = d_E; a.C = d_C;
    a.ldb = ldb; a.lde = lde; a.ldc = ldc; a.N = N;
    call.rows([&](const sextans_engine *e, const int *perm) { launch_op<sx::kAttnForward>(op, e, a, perm, call.s); });
    return call.close(name);
}

template <class ET>
int spmm_edge_backward(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const ET *d_E, int64_t lde, const float *d_G,
                       int64_t ldg, float *d_dB, int64_t lddb, ET *d_dE, int64_t ldde, void *stream, const char *name) {
    if (!h || bad_op(op) || bad_n(N)) return SEXTANS_ERR_INVALID;
    if (bad_ld(ldb, N) || bad_ld(lde, N) || bad_ld(ldg, N) || bad_ld(lddb, N) || bad_ld(ldde, N)) return SEXTANS_ERR_INVALID;
    if (misaligned(d_B, d_E, d_G, d_dB, d_dE)) return SEXTANS_ERR_INVALID;
    if (!d_dB && !d_dE) return SEXTANS_ERR_INVALID;
    if (d_dB && op == SEXTANS_EDGE_COPY) return SEXTANS_ERR_INVALID;
    bool need_b = false, need_e = false;   // MUL: E for dB, B for dE; ADD_RELU: both for either; ADD and COPY: neither
    if (op == SEXTANS_EDGE_MUL) { need_e = d_dB != nullptr; need_b = d_dE != nullptr; }
    else if (op == SEXTANS_EDGE_ADD_RELU) need_b = need_e = true;
    PatternCall call{h};
    if (int rc = call.open(!d_G || (need_b && !d_B) || (need_e && !d_E), stream)) return rc;
    if (call.degenerate()) {   // (dE has no element)
        attention_fill(d_dB, h->K, N, lddb, 0.0f, call.s);
        return call.done();
    }
    if (int rc = call.tables(d_dB != nullptr)) return rc;
    sx::EdgeArgsT<ET> a{};
    a.B = d_B; a.E = d_E; a.G = d_G; a.dB = d_dB; a.dE = d_dE;
    a.ldb = ldb; a.lde = lde; a.ldg = ldg; a.lddb = lddb; a.ldde = ldde; a.N = N;
    if (d_dB) call.cols([&](const sextans_engine *e, const int *perm) { launch_op<sx::kAttnBackwardCols>(op, e, a, perm, call.s); });
    if (d_dE) call.rows([&](const sextans_engine *e, const int *perm) { launch_op<sx::kAttnBackwardRows>(op, e, a, perm, call.s); });
    return call.close(name);
}

}  // namespace
}  // namespace sxe
