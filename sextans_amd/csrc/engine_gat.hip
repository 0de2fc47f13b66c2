// engine_gat.hip -- fused graph attention (GAT) over the pattern of the CSR matrix on an engine handle (include/sextans_amd.h):
//   sextans_gat_attention_device            O = softmax(LeakyReLU(adst[r] + asrc[c] + bias) on A's pattern) V per head, and the rows' log-sum-exp
//   sextans_gat_attention_backward_device   dadst, dasrc, dV (and dbias) from O, lse and the upstream gradient: a row pass over A, a column pass over A^T
//   sextans_gat_attention_dropout_device / _dropout_backward_device   the same with dropout on the attention coefficients (dropout_hash.h)
// Kernels: gat_kernels.h (the additive score) on the row walking of pattern_pass.h; the entry points' frame: pattern_launch.h.  A's
// values are never read.
#include "gat_kernels.h"
#include "pattern_launch.h"

namespace sxe {
namespace {

// e: the engine whose CSR arrays and softmax tables the pass walks (the column pass: the companion).  The slot width follows dv alone:
// the smallest of 8 / 16 / 32 / 64 / 128 floats that holds it.  Entries in flight per slot (U), as measured: the forward
// keeps the dot-product kernels' 4 (2 at width 128) -- 8 was slower on config 4 -- and so forms the same batches, the same (m, Z, acc)
// bits; the backward passes hold one gathered row per entry instead of two and run twice as many, 4 (2 at width 128).
// COUPLING with AttnPass (tests/test_gat_attention_gpu.py, identity activation): at slope 1, d a_dst is rounding residue and is compared
// with the dot-product kernel's dQ[..., 0], which holds only while both make the same roundings -- the forward's U and batches as in
// engine_attention.hip, and in the row pass a slot adding its entries j, j + E, j + 2 E, .. one after the other (an order U does not
// change).  Retune either kernel's forward U or the walk's order and that comparison has to be looked at again.
template <int PASS, class Args>
void launch_pass(const sextans_engine *e, const Args &a, const int *perm, bool heads_inside, hipStream_t s) {
    constexpr bool DROP = std::is_same_v<Args, sx::GatDropArgs>;
    for_width(a.dv, [&](auto w) {
        using W = decltype(w);
        launch_pattern<sx::GatPass<PASS, W::T, W::P, W::k128 ? 2 : 4, DROP>>(e, a, perm, heads_inside, s);
    });
}

}  // namespace
}  // namespace sxe

using namespace sxe;

namespace {

// both entry points of a pass end here (drop == NULL: the plain one)
int gat_forward(sextans_handle_t h, int heads, int dv, float negative_slope, const float *d_adst, int64_t ldadst, const float *d_asrc, int64_t ldasrc,
                const float *d_V, int64_t ldv, const float *d_bias, float *d_O, int64_t ldo, float *d_lse, const sextans_dropout *drop, void *stream) {
    if (!h || heads < 1 || bad_dim(dv) || bad_slope(negative_slope)) return SEXTANS_ERR_INVALID;   // nothing here needs a device
    const Dropout mode = dropout_mode(drop);
    if (mode == Dropout::kInvalid) return SEXTANS_ERR_INVALID;
    if (mode == Dropout::kPlain) drop = nullptr;
    if (ldadst < heads || ldasrc < heads || bad_ld(ldv, (int64_t)heads * dv) || bad_ld(ldo, (int64_t)heads * dv)) return SEXTANS_ERR_INVALID;
    if (misaligned(d_adst, d_asrc, d_V, d_bias, d_O, d_lse)) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    if (int rc = call.open(!d_adst || !d_asrc || !d_V || !d_O || !d_lse, stream)) return rc;
    if (call.degenerate()) {   // every row is empty
        attention_fill(d_O, h->M, heads * dv, ldo, 0.0f, call.s);
        attention_fill(d_lse, h->M, heads, heads, -INFINITY, call.s);
        return call.done();
    }
    if (int rc = call.tables(false)) return rc;
    sx::GatArgs a{};
    a.adst = d_adst; a.asrc = d_asrc; a.V = d_V; a.bias = d_bias; a.out = d_O; a.out_lse = d_lse;
    a.ldadst = ldadst; a.ldasrc = ldasrc; a.ldv = ldv; a.ldo = ldo;
    a.H = heads; a.dv = dv; a.slope = negative_slope;
    with_dropout<sx::GatDropArgs>(a, drop, [&](const auto &args) {
        call.rows([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnForward>(e, args, perm, false, call.s); });
    });
    return call.close("gat_fused", drop != nullptr);
}

int gat_backward(sextans_handle_t h, int heads, int dv, float negative_slope, const float *d_adst, int64_t ldadst, const float *d_asrc, int64_t ldasrc,
                 const float *d_V, int64_t ldv, const float *d_bias, const float *d_O, int64_t ldo, const float *d_lse, const float *d_G, int64_t ldg,
                 float *d_delta, float *d_dadst, int64_t lddadst, float *d_dasrc, int64_t lddasrc, float *d_dV, int64_t lddv, float *d_dbias,
                 const sextans_dropout *drop, void *stream) {
    if (!h || heads < 1 || bad_dim(dv) || bad_slope(negative_slope)) return SEXTANS_ERR_INVALID;
    const Dropout mode = dropout_mode(drop);
    if (mode == Dropout::kInvalid) return SEXTANS_ERR_INVALID;
    if (mode == Dropout::kPlain) drop = nullptr;
    const int64_t hdv = (int64_t)heads * dv;
    if (ldadst < heads || ldasrc < heads || lddadst < heads || lddasrc < heads || bad_ld(ldv, hdv) || bad_ld(ldo, hdv) || bad_ld(ldg, hdv) ||
        bad_ld(lddv, hdv))
        return SEXTANS_ERR_INVALID;
    if (misaligned(d_adst, d_asrc, d_V, d_bias, d_O, d_lse, d_G, d_delta, d_dadst, d_dasrc, d_dV, d_dbias)) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    if (int rc = call.open(!d_adst || !d_asrc || !d_V || !d_O || !d_lse || !d_G || !d_delta || !d_dadst || !d_dasrc || !d_dV, stream)) return rc;
    if (call.degenerate()) {
        attention_fill(d_delta, h->M, heads, heads, 0.0f, call.s);
        attention_fill(d_dadst, h->M, heads, lddadst, 0.0f, call.s);
        attention_fill(d_dasrc, h->K, heads, lddasrc, 0.0f, call.s);
        attention_fill(d_dV, h->K, (int)hdv, lddv, 0.0f, call.s);
        return call.done();
    }
    if (int rc = call.tables(true)) return rc;
    sx::GatArgs a{};
    a.adst = d_adst; a.asrc = d_asrc; a.V = d_V; a.bias = d_bias; a.O = d_O; a.lse = d_lse; a.G = d_G; a.delta = d_delta;
    a.out_delta = d_delta; a.dadst = d_dadst; a.dasrc = d_dasrc; a.dV = d_dV; a.dbias = d_dbias;
    a.ldadst = ldadst; a.ldasrc = ldasrc; a.ldv = ldv; a.ldo = ldo; a.ldg = ldg; a.lddadst = lddadst; a.lddasrc = lddasrc; a.lddv = lddv;
    a.H = heads; a.dv = dv; a.slope = negative_slope;
    with_dropout<sx::GatDropArgs>(a, drop, [&](const auto &args) {
        call.rows([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnBackwardRows>(e, args, perm, d_dbias != nullptr, call.s); });
        call.cols([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnBackwardCols>(e, args, perm, false, call.s); });
    });
    return call.close("gat_fused_backward", drop != nullptr);
}

}  // namespace

extern "C" {

int sextans_gat_attention_device(sextans_handle_t h, int heads, int dv, float negative_slope, const float *d_adst, int64_t ldadst, const float *d_asrc,
                                 int64_t ldasrc, const float *d_V, int64_t ldv, const float *d_bias, float *d_O, int64_t ldo, float *d_lse, void *stream) {
    return gat_forward(h, heads, dv, negative_slope, d_adst, ldadst, d_asrc, ldasrc, d_V, ldv, d_bias, d_O, ldo, d_lse, nullptr, stream);
}

int sextans_gat_attention_backward_device(sextans_handle_t h, int heads, int dv, float negative_slope, const float *d_adst, int64_t ldadst,
                                          const float *d_asrc, int64_t ldasrc, const float *d_V, int64_t ldv, const float *d_bias, const float *d_O,
                                          int64_t ldo, const float *d_lse, const float *d_G, int64_t ldg, float *d_delta, float *d_dadst, int64_t lddadst,
                                          float *d_dasrc, int64_t lddasrc, float *d_dV, int64_t lddv, float *d_dbias, void *stream) {
    return gat_backward(h, heads, dv, negative_slope, d_adst, ldadst, d_asrc, ldasrc, d_V, ldv, d_bias, d_O, ldo, d_lse, d_G, ldg, d_delta, d_dadst,
                        lddadst, d_dasrc, lddasrc, d_dV, lddv, d_dbias, nullptr, stream);
}

int sextans_gat_attention_dropout_device(sextans_handle_t h, int heads, int dv, float negative_slope, const float *d_adst, int64_t ldadst,
                                         const float *d_asrc, int64_t ldasrc, const float *d_V, int64_t ldv, const float *d_bias, float *d_O, int64_t ldo,
                                         float *d_lse, const sextans_dropout *drop, void *stream) {
    return gat_forward(h, heads, dv, negative_slope, d_adst, ldadst, d_asrc, ldasrc, d_V, ldv, d_bias, d_O, ldo, d_lse, drop, stream);
}

int sextans_gat_attention_dropout_backward_device(sextans_handle_t h, int heads, int dv, float negative_slope, const float *d_adst, int64_t ldadst,
                                                  const float *d_asrc, int64_t ldasrc, const float *d_V, int64_t ldv, const float *d_bias,
                                                  const float *d_O, int64_t ldo, const float *d_lse, const float *d_G, int64_t ldg, float *d_delta,
                                                  float *d_dadst, int64_t lddadst, float *d_dasrc, int64_t lddasrc, float *d_dV, int64_t lddv,
                                                  float *d_dbias, const sextans_dropout *drop, void *stream) {
    return gat_backward(h, heads, dv, negative_slope, d_adst, ldadst, d_asrc, ldasrc, d_V, ldv, d_bias, d_O, ldo, d_lse, d_G, ldg, d_delta, d_dadst,
                        lddadst, d_dasrc, lddasrc, d_dV, lddv, d_dbias, drop, stream);
}

}  // extern "C"
