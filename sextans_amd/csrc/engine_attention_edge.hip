// engine_attention_edge.hip -- the fused attention with a feature vector per stored entry on the key and on the value side
// (include/sextans_amd.h):
//   sextans_attention_edge_device            s_e = scale * (<Q[r], K[c] + Ek[e]> + bias_e);  O[r] = sum_e softmax_e(s) (V[c] + Ev[e])
//   sextans_attention_edge_backward_device   dQ, dK, dV, dEk, dEv (and dbias): a row pass over A, a column pass over A^T
// Passes: the EDGE variant of attention_kernels.h (AttnEdgePass), with and without dropout, in a translation unit of its own so that the
// build stays parallel; the kernels of engine_attention.hip are not touched.  The entry points' frame: pattern_launch.h.
// Ek == NULL and Ev == NULL: the plain entries serve the call.
#include "attention_kernels.h"
#include "pattern_launch.h"

namespace sxe {
namespace {

// Entries in flight per slot (U) as in engine_attention.hip: the forward 4, the backward passes 2; half of that at width 128.
template <int PASS, class Args>
void launch_pass(const sextans_engine *e, const Args &a, const int *perm, bool heads_inside, hipStream_t s) {
    constexpr bool F = PASS == sx::kAttnForward, DROP = std::is_same_v<Args, sx::AttnEdgeDropArgs>;
    for_width(a.d > a.dv ? a.d : a.dv, [&](auto w) {
        using W = decltype(w);
        launch_pattern<sx::AttnEdgePass<PASS, W::T, W::P, W::k128 ? (F ? 2 : 1) : (F ? 4 : 2), DROP>>(e, a, perm, heads_inside, s);
    });
}

// what both entries check before the handle's state: dimensions, dropout, every leading dimension of the forward's operands
int check_common(sextans_handle_t h, int heads, int d, int dv, const sextans_dropout *drop, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldek,
                 int64_t ldev, int64_t ldo) {
    if (!h || heads < 1 || bad_dim(d) || bad_dim(dv)) return SEXTANS_ERR_INVALID;
    if (dropout_mode(drop) == Dropout::kInvalid) return SEXTANS_ERR_INVALID;
    const int64_t hd = (int64_t)heads * d, hdv = (int64_t)heads * dv;
    if (bad_ld(ldq, hd) || bad_ld(ldk, hd) || bad_ld(ldv, hdv) || bad_ld(ldek, hd) || bad_ld(ldev, hdv) || bad_ld(ldo, hdv)) return SEXTANS_ERR_INVALID;
    return SEXTANS_OK;
}

}  // namespace
}  // namespace sxe

using namespace sxe;

extern "C" {

int sextans_attention_edge_device(sextans_handle_t h, int heads, int d, int dv, float scale, const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk,
                                  const float *d_V, int64_t ldv, const float *d_Ek, int64_t ldek, const float *d_Ev, int64_t ldev, const float *d_bias,
                                  float *d_O, int64_t ldo, float *d_lse, const sextans_dropout *drop, void *stream) {
    if (int rc = check_common(h, heads, d, dv, drop, ldq, ldk, ldv, ldek, ldev, ldo)) return rc;   // nothing here needs a device
    if (dropout_mode(drop) == Dropout::kPlain) drop = nullptr;
    if (misaligned(d_Q, d_K, d_V, d_Ek, d_Ev, d_bias, d_O, d_lse)) return SEXTANS_ERR_INVALID;
    if (!d_Ek && !d_Ev) return sextans_attention_dropout_device(h, heads, d, dv, scale, d_Q, ldq, d_K, ldk, d_V, ldv, d_bias, d_O, ldo, d_lse, drop, stream);
    PatternCall call{h};
    if (int rc = call.open(!d_Q || !d_K || !d_V || !d_O || !d_lse, stream)) return rc;
    if (call.degenerate()) {   // every row is empty
        attention_fill(d_O, h->M, heads * dv, ldo, 0.0f, call.s);
        attention_fill(d_lse, h->M, heads, heads, -INFINITY, call.s);
        return call.done();
    }
    if (int rc = call.tables(false)) return rc;
    sx::AttnEdgeArgs a{};
    a.Q = d_Q; a.K = d_K; a.V = d_V; a.bias = d_bias; a.out = d_O; a.out_lse = d_lse;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
    a.H = heads; a.d = d; a.dv = dv; a.scale = scale;
    a.Ek = d_Ek; a.Ev = d_Ev; a.ldek = ldek; a.ldev = ldev;
    with_dropout<sx::AttnEdgeDropArgs>(a, drop, [&](const auto &args) {
        call.rows([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnForward>(e, args, perm, false, call.s); });
    });
    return call.close("attention_edge_fused", drop != nullptr);
}

int sextans_attention_edge_backward_device(sextans_handle_t h, int heads, int d, int dv, float scale, const float *d_Q, int64_t ldq, const float *d_K,
                                           int64_t ldk, const float *d_V, int64_t ldv, const float *d_Ek, int64_t ldek, const float *d_Ev, int64_t ldev,
                                           const float *d_bias, const float *d_O, int64_t ldo, const float *d_lse, const float *d_G, int64_t ldg,
                                           float *d_delta, float *d_dQ, int64_t lddq, float *d_dK, int64_t lddk, float *d_dV, int64_t lddv, float *d_dEk,
                                           int64_t lddek, float *d_dEv, int64_t lddev, float *d_dbias, const sextans_dropout *drop, void *stream) {
    if (int rc = check_common(h, heads, d, dv, drop, ldq, ldk, ldv, ldek, ldev, ldo)) return rc;
    if (dropout_mode(drop) == Dropout::kPlain) drop = nullptr;
    const int64_t hd = (int64_t)heads * d, hdv = (int64_t)heads * dv;
    if (bad_ld(ldg, hdv) || bad_ld(lddq, hd) || bad_ld(lddk, hd) || bad_ld(lddv, hdv) || bad_ld(lddek, hd) || bad_ld(lddev, hdv)) return SEXTANS_ERR_INVALID;
    if (misaligned(d_Q, d_K, d_V, d_Ek, d_Ev, d_bias, d_O, d_lse, d_G, d_delta, d_dQ, d_dK, d_dV, d_dEk, d_dEv, d_dbias)) return SEXTANS_ERR_INVALID;
    if ((d_dEk && !d_Ek) || (d_dEv && !d_Ev)) return SEXTANS_ERR_INVALID;   // a gradient for an absent E
    if (d_dEk && d_dEk == d_dEv && (d != dv || lddek != lddev)) return SEXTANS_ERR_INVALID;   // (both E are present: the line above)
    if (!d_Ek && !d_Ev)
        return sextans_attention_dropout_backward_device(h, heads, d, dv, scale, d_Q, ldq, d_K, ldk, d_V, ldv, d_bias, d_O, ldo, d_lse, d_G, ldg, d_delta,
                                                         d_dQ, lddq, d_dK, lddk, d_dV, lddv, d_dbias, drop, stream);
    PatternCall call{h};
    if (int rc = call.open(!d_Q || !d_K || !d_V || !d_O || !d_lse || !d_G || !d_delta || !d_dQ || !d_dK || !d_dV, stream)) return rc;
    if (call.degenerate()) {   // (dEk and dEv have no element)
        attention_fill(d_delta, h->M, heads, heads, 0.0f, call.s);
        attention_fill(d_dQ, h->M, (int)hd, lddq, 0.0f, call.s);
        attention_fill(d_dK, h->K, (int)hd, lddk, 0.0f, call.s);
        attention_fill(d_dV, h->K, (int)hdv, lddv, 0.0f, call.s);
        return call.done();
    }
    if (int rc = call.tables(true)) return rc;
    sx::AttnEdgeArgs a{};
    a.Q = d_Q; a.K = d_K; a.V = d_V; a.bias = d_bias; a.O = d_O; a.lse = d_lse; a.G = d_G; a.delta = d_delta;
    a.out_delta = d_delta; a.dQ = d_dQ; a.dK = d_dK; a.dV = d_dV; a.dbias = d_dbias;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.ldg = ldg; a.lddq = lddq; a.lddk = lddk; a.lddv = lddv;
    a.H = heads; a.d = d; a.dv = dv; a.scale = scale;
    a.Ek = d_Ek; a.Ev = d_Ev; a.dEk = d_dEk; a.dEv = d_dEv; a.ldek = ldek; a.ldev = ldev; a.lddek = lddek; a.lddev = lddev;
    with_dropout<sx::AttnEdgeDropArgs>(a, drop, [&](const auto &args) {
        call.rows([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnBackwardRows>(e, args, perm, d_dbias != nullptr, call.s); });
        call.cols([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnBackwardCols>(e, args, perm, false, call.s); });
    });
    return call.close("attention_edge_fused_backward", drop != nullptr);
}

}  // extern "C"
