// engine_edge.hip -- SpMM with a feature vector per stored entry over the CSR pattern on an engine handle (include/sextans_amd.h):
//   sextans_spmm_edge_device_rm            C[r, :] = sum over row r's entries of B[c, :] (op) E[e, :]   (mul / add / relu(add) / copy)
//   sextans_spmm_edge_backward_device_rm   dB and dE from the upstream gradient: a column pass over A^T, a row pass over A
// Kernels: spmm_edge_kernels.h on the row walking of pattern_pass.h.  Tables as in engine_reduce.hip: the row softmax's of this
// engine for the forward and the row pass, those of the companion engine that holds A^T for the column pass.  Only the pattern is read:
// neither the engine's values nor any of its packed forms is read or touched.
#include "pattern_launch.h"
#include "spmm_edge_kernels.h"

namespace sxe {
namespace {

// e: the engine whose CSR arrays and softmax tables the pass walks (the column pass: the companion).  N is cut into tiles of the smallest
// of 8 / 16 / 32 / 64 / 128 floats that holds min(N, 128); the last tile may be partial; the tiles sit in the grid in every pass (the row
// pass too: an (entry, tile) belongs to one slot).  Entries in flight per slot (U): the reduce forward's 4 (2 at width 128) -- an entry
// costs up to two loads of a tile's pieces; untuned.
template <int PASS, int OP>
void launch_pass(const sextans_engine *e, const sx::EdgeArgs &a, const int *perm, hipStream_t s) {
    for_width(a.N, [&](auto w) {
        using W = decltype(w);
        launch_pattern<sx::EdgePass<PASS, OP, W::T, W::P, W::k128 ? 2 : 4>>(e, tiled<W>(a), perm, false, s);
    });
}

template <int PASS>
void launch_op(int op, const sextans_engine *e, const sx::EdgeArgs &a, const int *perm, hipStream_t s) {
    if (op == SEXTANS_EDGE_MUL) launch_pass<PASS, sx::kEdgeMul>(e, a, perm, s);
    else if (op == SEXTANS_EDGE_ADD) launch_pass<PASS, sx::kEdgeAdd>(e, a, perm, s);
    else if (op == SEXTANS_EDGE_ADD_RELU) launch_pass<PASS, sx::kEdgeAddRelu>(e, a, perm, s);
    else if constexpr (PASS != sx::kAttnBackwardCols) launch_pass<PASS, sx::kEdgeCopy>(e, a, perm, s);   // (COPY has no dB)
}

bool bad_op(int op) { return op < SEXTANS_EDGE_MUL || op > SEXTANS_EDGE_COPY; }

}  // namespace
}  // namespace sxe

using namespace sxe;

extern "C" {

int sextans_spmm_edge_device_rm(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const float *d_E, int64_t lde,
                                float *d_C, int64_t ldc, void *stream) {
    if (!h || bad_op(op) || bad_n(N)) return SEXTANS_ERR_INVALID;   // nothing here needs a device
    if (bad_ld(ldb, N) || bad_ld(lde, N) || bad_ld(ldc, N)) return SEXTANS_ERR_INVALID;
    if (misaligned(d_B, d_E, d_C)) return SEXTANS_ERR_INVALID;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    if (h->nnz > INT32_MAX) return SEXTANS_ERR_INVALID;
    if (h->nnz > 0 && ((!d_B && op != SEXTANS_EDGE_COPY) || !d_E || !d_C)) return SEXTANS_ERR_INVALID;
    SX_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (h->M == 0 || h->nnz == 0) {   // every row is empty
        attention_fill(d_C, h->M, N, ldc, 0.0f, s);
        SX_HIP(hipGetLastError());
        return SEXTANS_OK;
    }
    if (int rc = ensure_softmax_tables(h, s)) return rc;
    sx::EdgeArgs a{};
    a.B = d_B; a.E = d_E; a.C = d_C;
    a.ldb = ldb; a.lde = lde; a.ldc = ldc; a.N = N;
    launch_op<sx::kAttnForward>(op, h, a, nullptr, s);
    SX_HIP(hipGetLastError());
    h->last_kernel = h->softmax.nchunks > 0 ? "spmm_edge+long_rows" : "spmm_edge";
    return SEXTANS_OK;
}

int sextans_spmm_edge_backward_device_rm(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const float *d_E, int64_t lde,
                                         const float *d_G, int64_t ldg, float *d_dB, int64_t lddb, float *d_dE, int64_t ldde, void *stream) {
    if (!h || bad_op(op) || bad_n(N)) return SEXTANS_ERR_INVALID;
    if (bad_ld(ldb, N) || bad_ld(lde, N) || bad_ld(ldg, N) || bad_ld(lddb, N) || bad_ld(ldde, N)) return SEXTANS_ERR_INVALID;
    if (misaligned(d_B, d_E, d_G, d_dB, d_dE)) return SEXTANS_ERR_INVALID;
    if (!d_dB && !d_dE) return SEXTANS_ERR_INVALID;
    if (d_dB && op == SEXTANS_EDGE_COPY) return SEXTANS_ERR_INVALID;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    if (h->nnz > INT32_MAX) return SEXTANS_ERR_INVALID;
    if (h->nnz > 0) {
        bool need_b = false, need_e = false;   // MUL: E for dB, B for dE; ADD_RELU: both for either; ADD and COPY: neither
        if (op == SEXTANS_EDGE_MUL) { need_e = d_dB != nullptr; need_b = d_dE != nullptr; }
        else if (op == SEXTANS_EDGE_ADD_RELU) need_b = need_e = true;
        if (!d_G || (need_b && !d_B) || (need_e && !d_E)) return SEXTANS_ERR_INVALID;
    }
    SX_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (h->M == 0 || h->nnz == 0) {   // (dE has no element)
        attention_fill(d_dB, h->K, N, lddb, 0.0f, s);
        SX_HIP(hipGetLastError());
        return SEXTANS_OK;
    }
    if (int rc = d_dB ? ensure_backward_tables(h, s) : ensure_softmax_tables(h, s)) return rc;
    sx::EdgeArgs a{};
    a.B = d_B; a.E = d_E; a.G = d_G; a.dB = d_dB; a.dE = d_dE;
    a.ldb = ldb; a.lde = lde; a.ldg = ldg; a.lddb = lddb; a.ldde = ldde; a.N = N;
    bool long_rows = false;
    if (d_dB) {
        launch_op<sx::kAttnBackwardCols>(op, h->tr, a, h->at.d_tperm, s);
        long_rows |= h->tr->softmax.nchunks > 0;
    }
    if (d_dE) {
        launch_op<sx::kAttnBackwardRows>(op, h, a, nullptr, s);
        long_rows |= h->softmax.nchunks > 0;
    }
    SX_HIP(hipGetLastError());
    h->last_kernel = long_rows ? "spmm_edge_backward+long_rows" : "spmm_edge_backward";
    return SEXTANS_OK;
}

}  // extern "C"
