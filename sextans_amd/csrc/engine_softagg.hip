// engine_softagg.hip -- softmax aggregation SpMM over the CSR matrix on an engine handle (include/sextans_amd.h):
//   sextans_spmm_softagg_device_rm            C[r, n] = sum_e softmax_e(t[n] p_e)[n] p_e over row r's messages p_e = val[e] * B[c, n], and lse
//   sextans_spmm_softagg_workspace_floats     the floats of workspace dt needs (dt_rows, then the chunk sums)
//   sextans_spmm_softagg_backward_device_rm   dB, dval and dt from C, lse and the upstream gradient: a column pass over A^T, a row pass
//                                             over A, the two-level dt sum
// Kernels: spmm_softagg_kernels.h on the row walking of pattern_pass.h; the entry points' frame: pattern_launch.h.  The values come
// through an explicit pointer (NULL: the engine's current ones); none of the engine's packed forms is read or touched.
#include "pattern_launch.h"
#include "spmm_softagg_kernels.h"

namespace sxe {
namespace {

// e: the engine whose CSR arrays and softmax tables the pass walks (the column pass: the companion).  N is cut into tiles of the smallest
// of 8 / 16 / 32 / 64 / 128 floats that holds min(N, 128); the last tile may be partial.  The 128-float tile is NOT capped as spmm_multi's
// is: three floats of state per column fit -- the forward takes 182 VGPRs, the row pass all 256, nothing spills or uses scratch
// (profiles/spmm_softagg_kernel_resources.txt).
// Entries in flight per slot (U), all UNTUNED -- no other value has been timed: the reduce family's 4 (2 at width 128) in the forward and
// the row pass (an entry costs one gathered B row), half of that in the column pass, where an entry costs three gathered rows (C, lse, G).
// The row pass keeps the dt sum whether or not dt is asked for (no compile-time variant): it is W registers, two VALU operations per
// float next to the exponential and the seven that q takes, and W shuffles per merge step; a variant without it would double the
// row-pass kernels for the call that wants dval alone -- the rare one, since a fixed temperature is what spmm / spmm_reduce already cover
// at t = 0 and t = +-inf.  The store is predicated on the workspace pointer.
template <int PASS>
void launch_pass(const sextans_engine *e, const sx::SoftaggArgs &a, const int *perm, bool tiles_inside, hipStream_t s) {
    for_width(a.N, [&](auto w) {
        using W = decltype(w);
        constexpr int U = (W::k128 ? 2 : 4) / (PASS == sx::kAttnBackwardCols ? 2 : 1);
        launch_pattern<sx::SoftaggPass<PASS, W::T, W::P, U>>(e, tiled<W>(a), perm, tiles_inside, s);
    });
}

}  // namespace
}  // namespace sxe

using namespace sxe;

extern "C" {

int sextans_spmm_softagg_device_rm(sextans_handle_t h, int N, const float *d_val, const float *d_B, int64_t ldb, const float *d_t, float *d_C,
                                   int64_t ldc, float *d_lse, int64_t ldlse, void *stream) {
    if (!h || bad_n(N)) return SEXTANS_ERR_INVALID;   // nothing here needs a device
    if (bad_ld(ldb, N) || bad_ld(ldc, N) || bad_ld(ldlse, N)) return SEXTANS_ERR_INVALID;
    if (misaligned(d_val, d_B, d_t, d_C, d_lse)) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    if (int rc = call.open(!d_B || !d_C, stream)) return rc;
    if (call.degenerate()) {   // every row is empty
        attention_fill(d_C, h->M, N, ldc, 0.0f, call.s);
        attention_fill(d_lse, h->M, N, ldlse, -INFINITY, call.s);
        return call.done();
    }
    if (int rc = call.tables(false)) return rc;
    sx::SoftaggArgs a{};
    a.val = d_val ? d_val : h->d_v; a.B = d_B; a.t = d_t; a.out = d_C; a.out_lse = d_lse;
    a.ldb = ldb; a.ldc = ldc; a.ldlse = ldlse; a.N = N;
    call.rows([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnForward>(e, a, perm, false, call.s); });
    return call.close("spmm_softagg");
}

int64_t sextans_spmm_softagg_workspace_floats(sextans_handle_t h, int N) {
    if (!h || bad_n(N)) return -(int64_t)SEXTANS_ERR_INVALID;
    if (!h->d_rp) return -(int64_t)SEXTANS_ERR_STATE;
    return (int64_t)h->M * N + chunks_of(h->M) * N;
}

int sextans_spmm_softagg_backward_device_rm(sextans_handle_t h, int N, const float *d_val, const float *d_B, int64_t ldb, const float *d_t,
                                            const float *d_C, int64_t ldc, const float *d_lse, int64_t ldlse, const float *d_G, int64_t ldg,
                                            float *d_dB, int64_t lddb, float *d_dval, float *d_dt, float *d_work, void *stream) {
    if (!h || bad_n(N)) return SEXTANS_ERR_INVALID;
    if (bad_ld(ldb, N) || bad_ld(ldc, N) || bad_ld(ldlse, N) || bad_ld(ldg, N) || bad_ld(lddb, N)) return SEXTANS_ERR_INVALID;
    if (misaligned(d_val, d_B, d_t, d_C, d_lse, d_G, d_dB, d_dval, d_dt, d_work)) return SEXTANS_ERR_INVALID;
    if (!d_dB && !d_dval && !d_dt) return SEXTANS_ERR_INVALID;   // nothing to compute
    if (d_dt && !d_work) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    if (int rc = call.open(!d_B || !d_C || !d_lse || !d_G, stream)) return rc;
    float *d_rows = d_dt ? d_work : nullptr;   // the workspace is written only for dt
    float *d_part = d_rows ? d_rows + (int64_t)h->M * N : nullptr;
    if (call.degenerate()) {   // (dval has no element)
        attention_fill(d_dB, h->K, N, lddb, 0.0f, call.s);
        attention_fill(d_rows, h->M, N, N, 0.0f, call.s);   // dt_rows and the chunk sums: what the passes would have left
        attention_fill(d_part, chunks_of(h->M), N, N, 0.0f, call.s);
        attention_fill(d_dt, 1, N, N, 0.0f, call.s);
        return call.done();
    }
    if (int rc = call.tables(d_dB != nullptr)) return rc;
    sx::SoftaggArgs a{};
    a.val = d_val ? d_val : h->d_v; a.B = d_B; a.t = d_t; a.C = d_C; a.lse = d_lse; a.G = d_G;
    a.dB = d_dB; a.dval = d_dval; a.dt_rows = d_rows;
    a.ldb = ldb; a.ldc = ldc; a.ldlse = ldlse; a.ldg = ldg; a.lddb = lddb; a.N = N;
    if (d_dB) call.cols([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnBackwardCols>(e, a, perm, false, call.s); });
    if (d_dval || d_dt) call.rows([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnBackwardRows>(e, a, perm, true, call.s); });
    if (d_dt) column_sum_two_level(d_rows, h->M, N, d_part, d_dt, call.s);
    return call.close("spmm_softagg_backward");
}

}  // extern "C"
