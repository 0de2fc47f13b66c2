// engine_edge_dot.hip -- the per-head dot product of both endpoints of every stored entry of the CSR pattern on an engine handle
// (include/sextans_amd.h):
//   sextans_edge_dot_device            S[e, h] = <X[r, h, :], Y[c, h, :]> for every stored entry e = (r, c): one launch for all heads, dealt
//                                      by non-zeros (edge_dot_kernels.h) over the SDDMM's row table
//   sextans_edge_dot_backward_device   dX and dY from the upstream gradient Gs of S.  No kernel of its own: dX is the WEIGHT-mode forward
//                                      of sextans_score_attention_device (S := Gs, V := Y), dY the WEIGHT-mode column pass of
//                                      sextans_score_attention_backward_device (S := Gs, G := X), called as they are -- their bits
// Only the pattern is read: neither the engine's values nor any of its packed forms is read or touched.
// 2 lane counts x 5 register depths of the X piece forward (10 kernels).
#include <cstring>

#include "edge_dot_kernels.h"
#include "pattern_launch.h"

namespace sxe {
namespace {

template <int LPR, int NCH>
void launch_dot_nch(dim3 grid, hipStream_t s, const sextans_engine *h, int heads, int d, const float *X, int64_t ldx, const float *Y, int64_t ldy,
                    float *S, int64_t lds) {
    hipLaunchKernelGGL((sx::edge_dot_forward<LPR, NCH>), grid, dim3(256), 0, s, (long long)h->nnz, h->d_rp, h->d_ci, h->d_sddmm_row0, heads, d, X,
                       (long long)ldx, Y, (long long)ldy, S, (long long)lds);
}
template <int LPR>
void launch_dot(int nch_cap, dim3 grid, hipStream_t s, const sextans_engine *h, int heads, int d, const float *X, int64_t ldx, const float *Y,
                int64_t ldy, float *S, int64_t lds) {
    switch (nch_cap) {
    case 1: launch_dot_nch<LPR, 1>(grid, s, h, heads, d, X, ldx, Y, ldy, S, lds); break;
    case 2: launch_dot_nch<LPR, 2>(grid, s, h, heads, d, X, ldx, Y, ldy, S, lds); break;
    case 4: launch_dot_nch<LPR, 4>(grid, s, h, heads, d, X, ldx, Y, ldy, S, lds); break;
    case 8: launch_dot_nch<LPR, 8>(grid, s, h, heads, d, X, ldx, Y, ldy, S, lds); break;
    default: launch_dot_nch<LPR, 0>(grid, s, h, heads, d, X, ldx, Y, ldy, S, lds); break;
    }
}

// the score pass's grid holds the heads (65535 at most), and the forward counts the pairs of a range in an int
inline bool bad_heads(int heads) { return heads < 1 || heads > kMaxTiles; }

}  // namespace
}  // namespace sxe

using namespace sxe;

extern "C" {

int sextans_edge_dot_device(sextans_handle_t h, int heads, int d, const float *d_X, int64_t ldx, const float *d_Y, int64_t ldy, float *d_S,
                            int64_t lds, void *stream) {
    if (!h || bad_heads(heads) || bad_dim(d)) return SEXTANS_ERR_INVALID;   // nothing here needs a device
    const int64_t hd = (int64_t)heads * d;
    if (bad_ld(ldx, hd) || bad_ld(ldy, hd) || lds < heads) return SEXTANS_ERR_INVALID;
    if (misaligned(d_X, d_Y, d_S)) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    if (int rc = call.open(!d_X || !d_Y || !d_S, stream)) return rc;
    if (call.degenerate()) return SEXTANS_OK;   // S has no element
    if (int rc = ensure_sddmm_rows(h, call.s)) return rc;
    const long long waves = (h->nnz + sx::kEdgeDotWaveEntries - 1) / sx::kEdgeDotWaveEntries;
    const dim3 grid((unsigned)((waves + 3) / 4));
    // sextans_sddmm_device_rm's choice at N = d: 4 lanes per pair (a 64-byte segment per request), 2 where 16 does not divide d; the X
    // piece is kept in registers up to 8 chunks
    const int lpr = (d / 4) % 4 == 0 ? 4 : 2;
    const int nch = d / (4 * lpr);
    const int nch_cap = nch <= 1 ? 1 : nch <= 2 ? 2 : nch <= 4 ? 4 : nch <= 8 ? 8 : 0;
    if (lpr == 4) launch_dot<4>(nch_cap, grid, call.s, h, heads, d, d_X, ldx, d_Y, ldy, d_S, lds);
    else launch_dot<2>(nch_cap, grid, call.s, h, heads, d, d_X, ldx, d_Y, ldy, d_S, lds);
    return call.close("edge_dot");
}

int sextans_edge_dot_backward_device(sextans_handle_t h, int heads, int d, const float *d_X, int64_t ldx, const float *d_Y, int64_t ldy,
                                     const float *d_Gs, int64_t ldgs, float *d_dX, int64_t lddx, float *d_dY, int64_t lddy, void *stream) {
    if (!h || bad_heads(heads) || bad_dim(d)) return SEXTANS_ERR_INVALID;
    // what the backward reads of the forward's operands: the OTHER endpoint of each gradient that is asked for
    if (!d_dY) d_X = nullptr;
    if (!d_dX) d_Y = nullptr;
    const int64_t hd = (int64_t)heads * d;
    if ((d_dY && bad_ld(ldx, hd)) || (d_dX && bad_ld(ldy, hd)) || ldgs < heads || bad_ld_of(d_dX, lddx, hd) || bad_ld_of(d_dY, lddy, hd))
        return SEXTANS_ERR_INVALID;
    if (misaligned(d_X, d_Y, d_Gs, d_dX, d_dY)) return SEXTANS_ERR_INVALID;
    if (!d_dX && !d_dY) return SEXTANS_ERR_INVALID;   // nothing to compute
    PatternCall call{h};
    if (int rc = call.open(!d_Gs || (d_dY && !d_X) || (d_dX && !d_Y), stream)) return rc;
    if (call.degenerate()) {   // every row and column is empty
        attention_fill(d_dX, h->M, (int)hd, lddx, 0.0f, call.s);
        attention_fill(d_dY, h->K, (int)hd, lddy, 0.0f, call.s);
        return call.done();
    }
    // Each pass is the score family's entry point itself: its tables, its launch, its bits.  A pass names itself in last_kernel.
    const auto long_rows = [&] { return std::strstr(h->last_kernel, "+long_rows") != nullptr; };
    if (d_dY) {   // over A^T: dY[c, h, :] = sum of Gs[e, h] X[r, h, :] (the WEIGHT column pass reads S and G alone: V is a placeholder)
        if (int rc = sextans_score_attention_backward_device(h, SEXTANS_SCORE_WEIGHT, heads, d, d_Gs, ldgs, d_X, ldx, nullptr, 0, nullptr, d_X, ldx,
                                                             nullptr, ldgs, d_dY, lddy, nullptr, stream))
            return rc;
        call.long_rows |= long_rows();
    }
    if (d_dX) {   // over A: dX[r, h, :] = sum of Gs[e, h] Y[c, h, :]
        if (int rc = sextans_score_attention_device(h, SEXTANS_SCORE_WEIGHT, heads, d, d_Gs, ldgs, d_Y, ldy, d_dX, lddx, nullptr, nullptr, stream))
            return rc;
        call.long_rows |= long_rows();
    }
    return call.close("edge_dot_backward");
}

}  // extern "C"
