// engine_reduce.hip -- max / min aggregation SpMM over the CSR matrix on an engine handle (include/sextans_amd.h):
//   sextans_spmm_reduce_device_rm            C[r, :] = max / min over row r's entries of val[e] * B[c, :], and the winning entries (arg)
//   sextans_spmm_reduce_backward_device_rm   dB and dval from arg and the upstream gradient: a column pass over A^T, a row pass over A
// Kernels: spmm_reduce_kernels.h on the row walking of pattern_pass.h.  Tables as in engine_attention.hip: the row softmax's of this
// engine for the forward and the row pass, those of the companion engine that holds A^T for the column pass.  The values come through
// an explicit pointer (NULL: the engine's current ones); none of the engine's packed forms is read or touched.
#include "pattern_launch.h"
#include "spmm_reduce_kernels.h"

namespace sxe {
namespace {

// e: the engine whose CSR arrays and softmax tables the pass walks (the column pass: the companion).  N is cut into tiles of the smallest
// of 8 / 16 / 32 / 64 / 128 floats that holds min(N, 128); the last tile may be partial.  Entries in flight per slot (U): the attention
// forward's 4 (2 at width 128) in every pass -- an entry costs one gathered row (the column pass: an arg and a G row).
template <int PASS, int OP>
void launch_pass(const sextans_engine *e, const sx::ReduceArgs &a, const int *perm, bool tiles_inside, hipStream_t s) {
    for_width(a.N, [&](auto w) {
        using W = decltype(w);
        launch_pattern<sx::ReducePass<PASS, OP, W::T, W::P, W::k128 ? 2 : 4>>(e, tiled<W>(a), perm, tiles_inside, s);
    });
}

}  // namespace
}  // namespace sxe

using namespace sxe;

extern "C" {

int sextans_spmm_reduce_device_rm(sextans_handle_t h, int op, int N, const float *d_val, const float *d_B, int64_t ldb, float *d_C, int64_t ldc,
                                  int32_t *d_arg, int64_t ldarg, void *stream) {
    if (!h || (op != SEXTANS_REDUCE_MAX && op != SEXTANS_REDUCE_MIN) || bad_n(N)) return SEXTANS_ERR_INVALID;   // nothing here needs a device
    if (bad_ld(ldb, N) || bad_ld(ldc, N) || bad_ld(ldarg, N)) return SEXTANS_ERR_INVALID;
    if (misaligned(d_val, d_B, d_C, d_arg)) return SEXTANS_ERR_INVALID;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    if (h->nnz > INT32_MAX) return SEXTANS_ERR_INVALID;
    if (h->nnz > 0 && (!d_B || !d_C)) return SEXTANS_ERR_INVALID;
    SX_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (h->M == 0 || h->nnz == 0) {   // every row is empty
        attention_fill(d_C, h->M, N, ldc, 0.0f, s);
        fill<int>(d_arg, h->M, N, ldarg, -1, s);
        SX_HIP(hipGetLastError());
        return SEXTANS_OK;
    }
    if (int rc = ensure_softmax_tables(h, s)) return rc;
    sx::ReduceArgs a{};
    a.val = d_val ? d_val : h->d_v; a.B = d_B; a.C = d_C; a.out_arg = d_arg;
    a.ldb = ldb; a.ldc = ldc; a.ldarg = ldarg; a.N = N;
    if (op == SEXTANS_REDUCE_MAX) launch_pass<sx::kAttnForward, sx::kReduceMax>(h, a, nullptr, false, s);
    else launch_pass<sx::kAttnForward, sx::kReduceMin>(h, a, nullptr, false, s);
    SX_HIP(hipGetLastError());
    h->last_kernel = h->softmax.nchunks > 0 ? "spmm_reduce+long_rows" : "spmm_reduce";
    return SEXTANS_OK;
}

int sextans_spmm_reduce_backward_device_rm(sextans_handle_t h, int N, const float *d_val, const float *d_B, int64_t ldb, const int32_t *d_arg,
                                           int64_t ldarg, const float *d_G, int64_t ldg, float *d_dB, int64_t lddb, float *d_dval, void *stream) {
    if (!h || bad_n(N)) return SEXTANS_ERR_INVALID;
    if (bad_ld(ldb, N) || bad_ld(ldarg, N) || bad_ld(ldg, N) || bad_ld(lddb, N)) return SEXTANS_ERR_INVALID;
    if (misaligned(d_val, d_B, d_arg, d_G, d_dB, d_dval)) return SEXTANS_ERR_INVALID;
    if (!d_dB && !d_dval) return SEXTANS_ERR_INVALID;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    if (h->nnz > INT32_MAX) return SEXTANS_ERR_INVALID;
    if (h->nnz > 0 && (!d_arg || !d_G || (d_dval && !d_B))) return SEXTANS_ERR_INVALID;
    SX_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (h->M == 0 || h->nnz == 0) {   // (dval has no element)
        attention_fill(d_dB, h->K, N, lddb, 0.0f, s);
        SX_HIP(hipGetLastError());
        return SEXTANS_OK;
    }
    if (int rc = d_dB ? ensure_backward_tables(h, s) : ensure_softmax_tables(h, s)) return rc;
    sx::ReduceArgs a{};
    a.val = d_val ? d_val : h->d_v; a.B = d_B; a.arg = d_arg; a.G = d_G; a.dB = d_dB; a.dval = d_dval;
    a.ldb = ldb; a.ldarg = ldarg; a.ldg = ldg; a.lddb = lddb; a.N = N;
    bool long_rows = false;
    if (d_dB) {
        launch_pass<sx::kAttnBackwardCols, 0>(h->tr, a, h->at.d_tperm, false, s);
        long_rows |= h->tr->softmax.nchunks > 0;
    }
    if (d_dval) {
        launch_pass<sx::kAttnBackwardRows, 0>(h, a, nullptr, true, s);
        long_rows |= h->softmax.nchunks > 0;
    }
    SX_HIP(hipGetLastError());
    h->last_kernel = long_rows ? "spmm_reduce_backward+long_rows" : "spmm_reduce_backward";
    return SEXTANS_OK;
}

}  // extern "C"
