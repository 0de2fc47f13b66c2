// engine_multi.hip -- several aggregations of the same messages in one pass over the CSR matrix on an engine handle
// (include/sextans_amd.h):
//   sextans_spmm_multi_device_rm            sum, sum of squares, max and min (with their args) over row r's entries of val[e] * B[c, :]
//   sextans_spmm_multi_backward_device_rm   dB and dval from the four upstream gradients and the args: one column pass over A^T, one row
//                                           pass over A
// Kernels: spmm_multi_kernels.h on the row walking of pattern_pass.h; the entry points' frame: pattern_launch.h.  The values come
// through an explicit pointer (NULL: the engine's current ones); none of the engine's packed forms is read or touched.
#include "pattern_launch.h"
#include "spmm_multi_kernels.h"

namespace sxe {
namespace {

// e: the engine whose CSR arrays and softmax tables the pass walks (the column pass: the companion).  N is cut into tiles of the smallest
// of 8 / 16 / 32 / 64 floats that holds min(N, kMaxTile); the last tile may be partial.  THIS FAMILY'S TILE IS CAPPED AT 64 FLOATS (for_width
// itself is as it was): the forward keeps 6 floats of state per column and the merge holds a second copy; with the 128-float tile the
// full forward takes all 256 VGPRs, spills two into AGPRs and runs one wavefront per SIMD (profiles/spmm_multi_kernel_resources.txt,
// DESIGN 4.18).  Entries in flight per slot (U): the reduce family's 4 in the forward and the row pass (one gathered B row per entry);
// half of that in the column pass, where an entry costs up to six gathered rows (four gradients, two args).  Untuned.
constexpr int kMaxTile = 64;

template <int PASS, int GROUPS>
void launch_groups(const sextans_engine *e, const sx::MultiArgs &a, const int *perm, bool tiles_inside, hipStream_t s) {
    for_width(a.N < kMaxTile ? a.N : kMaxTile, [&](auto w) {
        using W = decltype(w);
        constexpr int U = (W::k128 ? 2 : 4) / (PASS == sx::kAttnBackwardCols ? 2 : 1);
        if constexpr (4 * W::T * W::P <= kMaxTile) launch_pattern<sx::MultiPass<PASS, GROUPS, W::T, W::P, U>>(e, tiled<W>(a), perm, tiles_inside, s);
    });
}

template <int PASS>
void launch_pass(int groups, const sextans_engine *e, const sx::MultiArgs &a, const int *perm, bool tiles_inside, hipStream_t s) {
    if (groups == sx::kMultiMoments) launch_groups<PASS, sx::kMultiMoments>(e, a, perm, tiles_inside, s);
    else if (groups == sx::kMultiExtrema) launch_groups<PASS, sx::kMultiExtrema>(e, a, perm, tiles_inside, s);
    else launch_groups<PASS, sx::kMultiMoments | sx::kMultiExtrema>(e, a, perm, tiles_inside, s);
}

}  // namespace
}  // namespace sxe

using namespace sxe;

extern "C" {

int sextans_spmm_multi_device_rm(sextans_handle_t h, int N, const float *d_val, const float *d_B, int64_t ldb, const sextans_multi_out *out,
                                 void *stream) {
    if (!h || !out || bad_n(N) || too_many_tiles(N, kMaxTile)) return SEXTANS_ERR_INVALID;   // nothing here needs a device
    if (bad_ld(ldb, N) || bad_ld_of(out->d_sum, out->ld_sum, N) || bad_ld_of(out->d_sumsq, out->ld_sumsq, N) ||
        bad_ld_of(out->d_max, out->ld_max, N) || bad_ld_of(out->d_min, out->ld_min, N))
        return SEXTANS_ERR_INVALID;
    if ((out->d_argmax || out->d_argmin) && bad_ld(out->ld_arg, N)) return SEXTANS_ERR_INVALID;
    if (misaligned(d_val, d_B, out->d_sum, out->d_sumsq, out->d_max, out->d_min, out->d_argmax, out->d_argmin)) return SEXTANS_ERR_INVALID;
    if (!out->d_sum && !out->d_sumsq && !out->d_max && !out->d_min) return SEXTANS_ERR_INVALID;   // no output requested
    if ((out->d_argmax && !out->d_max) || (out->d_argmin && !out->d_min)) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    if (int rc = call.open(!d_B, stream)) return rc;
    if (call.degenerate()) {   // every row is empty
        attention_fill(out->d_sum, h->M, N, out->ld_sum, 0.0f, call.s);
        attention_fill(out->d_sumsq, h->M, N, out->ld_sumsq, 0.0f, call.s);
        attention_fill(out->d_max, h->M, N, out->ld_max, 0.0f, call.s);
        attention_fill(out->d_min, h->M, N, out->ld_min, 0.0f, call.s);
        fill<int>(out->d_argmax, h->M, N, out->ld_arg, -1, call.s);
        fill<int>(out->d_argmin, h->M, N, out->ld_arg, -1, call.s);
        return call.done();
    }
    if (int rc = call.tables(false)) return rc;
    sx::MultiArgs a{};
    a.val = d_val ? d_val : h->d_v; a.B = d_B; a.ldb = ldb; a.N = N;
    a.sum = out->d_sum; a.sumsq = out->d_sumsq; a.mx = out->d_max; a.mn = out->d_min;
    a.out_argmax = out->d_argmax; a.out_argmin = out->d_argmin;
    a.ld_sum = out->ld_sum; a.ld_sumsq = out->ld_sumsq; a.ld_max = out->ld_max; a.ld_min = out->ld_min; a.ld_arg = out->ld_arg;
    const int groups = ((a.sum || a.sumsq) ? sx::kMultiMoments : 0) | ((a.mx || a.mn) ? sx::kMultiExtrema : 0);
    call.rows([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnForward>(groups, e, a, perm, false, call.s); });
    return call.close("spmm_multi");
}

int sextans_spmm_multi_backward_device_rm(sextans_handle_t h, int N, const float *d_val, const float *d_B, int64_t ldb,
                                          const sextans_multi_grad *g, float *d_dB, int64_t lddb, float *d_dval, void *stream) {
    if (!h || !g || bad_n(N) || too_many_tiles(N, kMaxTile)) return SEXTANS_ERR_INVALID;
    if (bad_ld(ldb, N) || bad_ld(lddb, N) || bad_ld_of(g->d_gsum, g->ld_gsum, N) || bad_ld_of(g->d_gsumsq, g->ld_gsumsq, N) ||
        bad_ld_of(g->d_gmax, g->ld_gmax, N) || bad_ld_of(g->d_gmin, g->ld_gmin, N))
        return SEXTANS_ERR_INVALID;
    if ((g->d_argmax || g->d_argmin) && bad_ld(g->ld_arg, N)) return SEXTANS_ERR_INVALID;
    if (misaligned(d_val, d_B, g->d_gsum, g->d_gsumsq, g->d_gmax, g->d_gmin, g->d_argmax, g->d_argmin, d_dB, d_dval)) return SEXTANS_ERR_INVALID;
    if (!g->d_gsum && !g->d_gsumsq && !g->d_gmax && !g->d_gmin) return SEXTANS_ERR_INVALID;   // no gradient given
    if ((g->d_gmax && !g->d_argmax) || (g->d_gmin && !g->d_argmin)) return SEXTANS_ERR_INVALID;
    if (!d_dB && !d_dval) return SEXTANS_ERR_INVALID;
    if ((g->d_gsumsq || d_dval) && !d_B) return SEXTANS_ERR_INVALID;   // p_e and dval read B
    PatternCall call{h};
    if (int rc = call.open(false, stream)) return rc;   // (what is required is required by rule, above)
    if (call.degenerate()) {   // (dval has no element)
        attention_fill(d_dB, h->K, N, lddb, 0.0f, call.s);
        return call.done();
    }
    if (int rc = call.tables(d_dB != nullptr)) return rc;
    sx::MultiArgs a{};
    a.val = d_val ? d_val : h->d_v; a.B = d_B; a.ldb = ldb; a.N = N;
    a.gsum = g->d_gsum; a.gsumsq = g->d_gsumsq; a.gmax = g->d_gmax; a.gmin = g->d_gmin;
    a.argmax = g->d_argmax; a.argmin = g->d_argmin;
    a.ld_sum = g->ld_gsum; a.ld_sumsq = g->ld_gsumsq; a.ld_max = g->ld_gmax; a.ld_min = g->ld_gmin; a.ld_arg = g->ld_arg;
    a.dB = d_dB; a.dval = d_dval; a.lddb = lddb;
    const int groups = ((a.gsum || a.gsumsq) ? sx::kMultiMoments : 0) | ((a.gmax || a.gmin) ? sx::kMultiExtrema : 0);
    if (d_dB) call.cols([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnBackwardCols>(groups, e, a, perm, false, call.s); });
    if (d_dval) call.rows([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnBackwardRows>(groups, e, a, perm, true, call.s); });
    return call.close("spmm_multi_backward");
}

}  // extern "C"
