// engine_edge_multi.hip -- several aggregations of edge-feature messages in one pass over the CSR pattern on an engine handle
// (include/sextans_amd.h):
//   sextans_spmm_edge_multi_device_rm            sum, sum of squares, max and min (with their args) over row r's entries of
//                                                B[c, :] (op) E[e, :]   (mul / add / relu(add) / copy)
//   sextans_spmm_edge_multi_backward_device_rm   dB and dE from the four upstream gradients and the args: a column pass over A^T, a row
//                                                pass over A
// Kernels: spmm_edge_multi_kernels.h on the row walking of pattern_pass.h, instantiated one op per source (edge_multi_launch.h); the
// entry points' frame: pattern_launch.h.  Only the pattern is read: neither the engine's values nor any of its packed forms is read
// or touched.
#include "edge_multi_launch.h"

namespace sxe {
namespace {

void launch_op(int op, int pass, int groups, const sextans_engine *e, const sx::EdgeMultiArgs &a, const int *perm, hipStream_t s) {
    if (op == SEXTANS_EDGE_MUL) launch_edge_multi_mul(pass, groups, e, a, perm, s);
    else if (op == SEXTANS_EDGE_ADD) launch_edge_multi_add(pass, groups, e, a, perm, s);
    else if (op == SEXTANS_EDGE_ADD_RELU) launch_edge_multi_add_relu(pass, groups, e, a, perm, s);
    else launch_edge_multi_copy(pass, groups, e, a, perm, s);
}

bool bad_op(int op) { return op < SEXTANS_EDGE_MUL || op > SEXTANS_EDGE_COPY; }

}  // namespace
}  // namespace sxe

using namespace sxe;

extern "C" {

int sextans_spmm_edge_multi_device_rm(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const float *d_E, int64_t lde,
                                      const sextans_multi_out *out, void *stream) {
    if (!h || !out || bad_op(op) || bad_n(N) || too_many_tiles(N, kEdgeMultiMaxTile)) return SEXTANS_ERR_INVALID;   // nothing here needs a device
    if (bad_ld(ldb, N) || bad_ld(lde, N) || bad_ld_of(out->d_sum, out->ld_sum, N) || bad_ld_of(out->d_sumsq, out->ld_sumsq, N) ||
        bad_ld_of(out->d_max, out->ld_max, N) || bad_ld_of(out->d_min, out->ld_min, N))
        return SEXTANS_ERR_INVALID;
    if ((out->d_argmax || out->d_argmin) && bad_ld(out->ld_arg, N)) return SEXTANS_ERR_INVALID;
    if (misaligned(d_B, d_E, out->d_sum, out->d_sumsq, out->d_max, out->d_min, out->d_argmax, out->d_argmin)) return SEXTANS_ERR_INVALID;
    if (!out->d_sum && !out->d_sumsq && !out->d_max && !out->d_min) return SEXTANS_ERR_INVALID;   // no output requested
    if ((out->d_argmax && !out->d_max) || (out->d_argmin && !out->d_min)) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    if (int rc = call.open(!d_E || (!d_B && op != SEXTANS_EDGE_COPY), stream)) return rc;
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
    sx::EdgeMultiArgs a{};
    a.B = d_B; a.E = d_E; a.ldb = ldb; a.lde = lde; a.N = N;
    a.sum = out->d_sum; a.sumsq = out->d_sumsq; a.mx = out->d_max; a.mn = out->d_min;
    a.out_argmax = out->d_argmax; a.out_argmin = out->d_argmin;
    a.ld_sum = out->ld_sum; a.ld_sumsq = out->ld_sumsq; a.ld_max = out->ld_max; a.ld_min = out->ld_min; a.ld_arg = out->ld_arg;
    const int groups = ((a.sum || a.sumsq) ? sx::kMultiMoments : 0) | ((a.mx || a.mn) ? sx::kMultiExtrema : 0);
    call.rows([&](const sextans_engine *e, const int *perm) { launch_op(op, sx::kAttnForward, groups, e, a, perm, call.s); });
    return call.close("spmm_edge_multi");
}

int sextans_spmm_edge_multi_backward_device_rm(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const float *d_E, int64_t lde,
                                               const sextans_multi_grad *g, float *d_dB, int64_t lddb, float *d_dE, int64_t ldde, void *stream) {
    if (!h || !g || bad_op(op) || bad_n(N) || too_many_tiles(N, kEdgeMultiMaxTile)) return SEXTANS_ERR_INVALID;
    if (bad_ld(ldb, N) || bad_ld(lde, N) || bad_ld(lddb, N) || bad_ld(ldde, N) || bad_ld_of(g->d_gsum, g->ld_gsum, N) ||
        bad_ld_of(g->d_gsumsq, g->ld_gsumsq, N) || bad_ld_of(g->d_gmax, g->ld_gmax, N) || bad_ld_of(g->d_gmin, g->ld_gmin, N))
        return SEXTANS_ERR_INVALID;
    if ((g->d_argmax || g->d_argmin) && bad_ld(g->ld_arg, N)) return SEXTANS_ERR_INVALID;
    if (misaligned(d_B, d_E, g->d_gsum, g->d_gsumsq, g->d_gmax, g->d_gmin, g->d_argmax, g->d_argmin, d_dB, d_dE)) return SEXTANS_ERR_INVALID;
    if (!g->d_gsum && !g->d_gsumsq && !g->d_gmax && !g->d_gmin) return SEXTANS_ERR_INVALID;   // no gradient given
    if ((g->d_gmax && !g->d_argmax) || (g->d_gmin && !g->d_argmin)) return SEXTANS_ERR_INVALID;
    if (!d_dB && !d_dE) return SEXTANS_ERR_INVALID;
    if (d_dB && op == SEXTANS_EDGE_COPY) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    // required by rule; a kernel reads an operand only where its formula does
    if (int rc = call.open(!d_E || (!d_B && op != SEXTANS_EDGE_COPY), stream)) return rc;
    if (call.degenerate()) {   // (dE has no element)
        attention_fill(d_dB, h->K, N, lddb, 0.0f, call.s);
        return call.done();
    }
    if (int rc = call.tables(d_dB != nullptr)) return rc;
    sx::EdgeMultiArgs a{};
    a.B = d_B; a.E = d_E; a.ldb = ldb; a.lde = lde; a.N = N;
    a.gsum = g->d_gsum; a.gsumsq = g->d_gsumsq; a.gmax = g->d_gmax; a.gmin = g->d_gmin;
    a.argmax = g->d_argmax; a.argmin = g->d_argmin;
    a.ld_sum = g->ld_gsum; a.ld_sumsq = g->ld_gsumsq; a.ld_max = g->ld_gmax; a.ld_min = g->ld_gmin; a.ld_arg = g->ld_arg;
    a.dB = d_dB; a.dE = d_dE; a.lddb = lddb; a.ldde = ldde;
    const int groups = ((a.gsum || a.gsumsq) ? sx::kMultiMoments : 0) | ((a.gmax || a.gmin) ? sx::kMultiExtrema : 0);
    if (d_dB) call.cols([&](const sextans_engine *e, const int *perm) { launch_op(op, sx::kAttnBackwardCols, groups, e, a, perm, call.s); });
    if (d_dE) call.rows([&](const sextans_engine *e, const int *perm) { launch_op(op, sx::kAttnBackwardRows, groups, e, a, perm, call.s); });
    return call.close("spmm_edge_multi_backward");
}

}  // extern "C"
