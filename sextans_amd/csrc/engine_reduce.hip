// engine_reduce.hip -- max / min aggregation SpMM over the CSR matrix on an engine handle (include/sextans_amd.h):
//   sextans_spmm_reduce_device_rm            C[r, :] = max / min over row r's entries of val[e] * B[c, :], and the winning entries (arg)
//   sextans_spmm_reduce_backward_device_rm   dB and dval from arg and the upstream gradient: a column pass over A^T, a row pass over A
// Kernels: spmm_reduce_kernels.h on the row walking of pattern_pass.h; the entry points' frame: pattern_launch.h.  The values come
// through an explicit pointer (NULL: the engine's current ones); none of the engine's packed forms is read or touched.
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
    PatternCall call{h};
    if (int rc = call.open(!d_B || !d_C, stream)) return rc;
    if (call.degenerate()) {   // every row is empty
        attention_fill(d_C, h->M, N, ldc, 0.0f, call.s);
        fill<int>(d_arg, h->M, N, ldarg, -1, call.s);
        return call.done();
    }
    if (int rc = call.tables(false)) return rc;
    sx::ReduceArgs a{};
    a.val = d_val ? d_val : h->d_v; a.B = d_B; a.C = d_C; a.out_arg = d_arg;
    a.ldb = ldb; a.ldc = ldc; a.ldarg = ldarg; a.N = N;
    call.rows([&](const sextans_engine *e, const int *perm) {
        if (op == SEXTANS_REDUCE_MAX) launch_pass<sx::kAttnForward, sx::kReduceMax>(e, a, perm, false, call.s);
        else launch_pass<sx::kAttnForward, sx::kReduceMin>(e, a, perm, false, call.s);
    });
    return call.close("spmm_reduce");
}

int sextans_spmm_reduce_backward_device_rm(sextans_handle_t h, int N, const float *d_val, const float *d_B, int64_t ldb, const int32_t *d_arg,
                                           int64_t ldarg, const float *d_G, int64_t ldg, float *d_dB, int64_t lddb, float *d_dval, void *stream) {
    if (!h || bad_n(N)) return SEXTANS_ERR_INVALID;
    if (bad_ld(ldb, N) || bad_ld(ldarg, N) || bad_ld(ldg, N) || bad_ld(lddb, N)) return SEXTANS_ERR_INVALID;
    if (misaligned(d_val, d_B, d_arg, d_G, d_dB, d_dval)) return SEXTANS_ERR_INVALID;
    if (!d_dB && !d_dval) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    if (int rc = call.open(!d_arg || !d_G || (d_dval && !d_B), stream)) return rc;
    if (call.degenerate()) {   // (dval has no element)
        attention_fill(d_dB, h->K, N, lddb, 0.0f, call.s);
        return call.done();
    }
    if (int rc = call.tables(d_dB != nullptr)) return rc;
    sx::ReduceArgs a{};
    a.val = d_val ? d_val : h->d_v; a.B = d_B; a.arg = d_arg; a.G = d_G; a.dB = d_dB; a.dval = d_dval;
    a.ldb = ldb; a.ldarg = ldarg; a.ldg = ldg; a.lddb = lddb; a.N = N;
    if (d_dB) call.cols([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnBackwardCols, 0>(e, a, perm, false, call.s); });
    if (d_dval) call.rows([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnBackwardRows, 0>(e, a, perm, true, call.s); });
    return call.close("spmm_reduce_backward");
}

}  // extern "C"
