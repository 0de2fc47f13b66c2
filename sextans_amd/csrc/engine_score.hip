// engine_score.hip -- attention over the pattern of the CSR matrix from caller-supplied per-(entry, head) scores on an engine handle
// (include/sextans_amd.h):
//   sextans_score_attention_device            SOFTMAX: O = softmax(S on A's pattern) V per head and the rows' log-sum-exp; WEIGHT: O = S V per head
//   sextans_score_attention_backward_device   dS (nnz x heads, stored per element) and dV from the upstream gradient: a row pass over A, a
//                                             column pass over A^T; either may be skipped
// Kernels: score_kernels.h on the row walking of pattern_pass.h; the entry points' frame: pattern_launch.h.  A's values are never read.
#include "score_kernels.h"
#include "pattern_launch.h"

namespace sxe {
namespace {

// e: the engine whose CSR arrays and softmax tables the pass walks (the column pass: the companion).  The slot width follows dv alone.
// Entries in flight per slot (U): the forward keeps the GAT forward's 4 (2 at width 128).
// COUPLING with GatPass (tests/test_score_attention_gpu.py, the bit anchor): fed S[e, h] = the score GAT computes, O, lse and dV are
// compared BIT FOR BIT with sextans_gat_attention_device / _backward_device.  The online softmax takes its maximum per batch of U
// entries, so that holds only while both forwards form the same batches -- the U of engine_gat.hip's forward -- and while the column
// pass's slot adds its entries j, j + E, j + 2 E, .. one after the other (an order U does not change).  Retune either forward's U and
// that comparison has to be looked at again.
// The backward passes: 4 (2 at width 128) as GAT's, UNTUNED -- nobody has measured another value on this family.
template <int PASS, int MODE, class Args>
void launch_pass(const sextans_engine *e, const Args &a, const int *perm, hipStream_t s) {
    constexpr bool DROP = std::is_same_v<Args, sx::ScoreDropArgs>;
    if constexpr (MODE == sx::kScoreSoftmax || !DROP) {
        for_width(a.dv, [&](auto w) {
            using W = decltype(w);
            launch_pattern<sx::ScorePass<PASS, MODE, W::T, W::P, W::k128 ? 2 : 4, DROP>>(e, a, perm, false, s);
        });
    }
}
// WEIGHT never takes dropout (the entry points refuse it): only the plain args reach its instantiations
template <int PASS, class Args>
void launch_mode(int mode, const sextans_engine *e, const Args &a, const int *perm, hipStream_t s) {
    if (mode == sx::kScoreSoftmax) launch_pass<PASS, sx::kScoreSoftmax>(e, a, perm, s);
    else launch_pass<PASS, sx::kScoreWeight>(e, a, perm, s);
}

inline bool bad_mode(int mode) { return mode != SEXTANS_SCORE_SOFTMAX && mode != SEXTANS_SCORE_WEIGHT; }
inline const char *base_name(int mode, bool backward) {
    if (mode == SEXTANS_SCORE_SOFTMAX) return backward ? "score_softmax_fused_backward" : "score_softmax_fused";
    return backward ? "score_weight_fused_backward" : "score_weight_fused";
}

}  // namespace
}  // namespace sxe

using namespace sxe;

extern "C" {

int sextans_score_attention_device(sextans_handle_t h, int mode, int heads, int dv, const float *d_S, int64_t lds, const float *d_V, int64_t ldv,
                                   float *d_O, int64_t ldo, float *d_lse, const sextans_dropout *drop, void *stream) {
    if (!h || bad_mode(mode) || heads < 1 || bad_dim(dv)) return SEXTANS_ERR_INVALID;   // nothing here needs a device
    const bool soft = mode == SEXTANS_SCORE_SOFTMAX;
    const Dropout dmode = dropout_mode(drop);
    if (dmode == Dropout::kInvalid || (dmode == Dropout::kActive && !soft)) return SEXTANS_ERR_INVALID;   // dropout in WEIGHT mode
    if (dmode == Dropout::kPlain) drop = nullptr;
    if (lds < heads || bad_ld(ldv, (int64_t)heads * dv) || bad_ld(ldo, (int64_t)heads * dv)) return SEXTANS_ERR_INVALID;
    if (misaligned(d_S, d_V, d_O, d_lse)) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    if (int rc = call.open(!d_S || !d_V || !d_O || (soft && !d_lse), stream)) return rc;
    if (call.degenerate()) {   // every row is empty
        attention_fill(d_O, h->M, heads * dv, ldo, 0.0f, call.s);
        if (soft) attention_fill(d_lse, h->M, heads, heads, -INFINITY, call.s);
        return call.done();
    }
    if (int rc = call.tables(false)) return rc;
    sx::ScoreArgs a{};
    a.S = d_S; a.V = d_V; a.out = d_O; a.out_lse = d_lse;
    a.lds = lds; a.ldv = ldv; a.ldo = ldo;
    a.H = heads; a.dv = dv;
    with_dropout<sx::ScoreDropArgs>(a, drop, [&](const auto &args) {
        call.rows([&](const sextans_engine *e, const int *perm) { launch_mode<sx::kAttnForward>(mode, e, args, perm, call.s); });
    });
    return call.close(base_name(mode, false), drop != nullptr);
}

int sextans_score_attention_backward_device(sextans_handle_t h, int mode, int heads, int dv, const float *d_S, int64_t lds, const float *d_V,
                                            int64_t ldv, const float *d_O, int64_t ldo, const float *d_lse, const float *d_G, int64_t ldg,
                                            float *d_dS, int64_t ldds, float *d_dV, int64_t lddv, const sextans_dropout *drop, void *stream) {
    if (!h || bad_mode(mode) || heads < 1 || bad_dim(dv)) return SEXTANS_ERR_INVALID;
    const bool soft = mode == SEXTANS_SCORE_SOFTMAX;
    const Dropout dmode = dropout_mode(drop);
    if (dmode == Dropout::kInvalid || (dmode == Dropout::kActive && !soft)) return SEXTANS_ERR_INVALID;
    if (dmode == Dropout::kPlain) drop = nullptr;
    const int64_t hdv = (int64_t)heads * dv;
    // (WEIGHT reads no O: its ldo is not looked at)
    if (lds < heads || ldds < heads || bad_ld(ldv, hdv) || (soft && bad_ld(ldo, hdv)) || bad_ld(ldg, hdv) || bad_ld(lddv, hdv)) return SEXTANS_ERR_INVALID;
    if (misaligned(d_S, d_V, d_O, d_lse, d_G, d_dS, d_dV)) return SEXTANS_ERR_INVALID;
    if (!h->d_rp) return SEXTANS_ERR_STATE;            // this family documents "nothing to compute" after STATE: both stay here
    if (!d_dS && !d_dV) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    if (int rc = call.open(!d_S || !d_V || !d_G || (soft && (!d_O || !d_lse)), stream)) return rc;
    if (call.degenerate()) {   // (no entries: dS has no element)
        attention_fill(d_dV, h->K, (int)hdv, lddv, 0.0f, call.s);
        return call.done();
    }
    if (int rc = call.tables(d_dV != nullptr)) return rc;
    sx::ScoreArgs a{};
    a.S = d_S; a.V = d_V; a.O = d_O; a.lse = d_lse; a.G = d_G; a.dS = d_dS; a.dV = d_dV;
    a.lds = lds; a.ldv = ldv; a.ldo = ldo; a.ldg = ldg; a.ldds = ldds; a.lddv = lddv;
    a.H = heads; a.dv = dv;
    with_dropout<sx::ScoreDropArgs>(a, drop, [&](const auto &args) {
        if (d_dS) call.rows([&](const sextans_engine *e, const int *perm) { launch_mode<sx::kAttnBackwardRows>(mode, e, args, perm, call.s); });
        if (d_dV) call.cols([&](const sextans_engine *e, const int *perm) { launch_mode<sx::kAttnBackwardCols>(mode, e, args, perm, call.s); });
    });
    return call.close(base_name(mode, true), drop != nullptr);
}

}  // extern "C"
