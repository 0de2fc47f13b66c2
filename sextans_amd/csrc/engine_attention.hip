// engine_attention.hip -- fused multi-head attention over the pattern of the CSR matrix on an engine handle (include/sextans_amd.h):
//   sextans_attention_device            O = softmax(scale * (Q K^T + bias) on A's pattern) V per head, and the rows' log-sum-exp
//   sextans_attention_backward_device   dQ, dK, dV (and dbias) from O, lse and the upstream gradient: a row pass over A, a column pass over A^T
//   sextans_attention_dropout_device / _dropout_backward_device   the same with dropout on the attention coefficients (dropout_hash.h)
//   sextans_dropout_mask_device, sextans_dropout_keep_host        the mask itself: nnz * heads multipliers on the device, keep flags on the host
// Passes: attention_kernels.h on the row walking of pattern_pass.h; the entry points' frame: pattern_launch.h.  No table of its own,
// and A's values are never read.
#include "attention_kernels.h"
#include "pattern_launch.h"

namespace sx {

// out[i] = the dropout multiplier of (entry i / heads, head i % heads): the hash's counter is i itself
__global__ __launch_bounds__(256) void dropout_mask(DropArgs d, long long n, float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = dropout_u32(drop_key(d), (uint64_t)i, 1u, 0u) >= d.thresh ? d.inv_keep : 0.0f;
}

}  // namespace sx

namespace sxe {

// (declared in engine_state.h: the other four families fill their degenerate calls' outputs with it too)
void attention_fill(float *out, int64_t rows, int cols, int64_t ld, float value, hipStream_t s) {
    fill<float>(out, rows, cols, ld, value, s);
}

namespace {

int check_dims(sextans_handle_t h, int heads, int d, int dv) {
    if (!h || heads < 1 || bad_dim(d) || bad_dim(dv)) return SEXTANS_ERR_INVALID;
    return SEXTANS_OK;
}

// e: the engine whose CSR arrays and softmax tables the pass walks (the column pass: the companion).  One register width serves both
// head dimensions: the smallest of 8 / 16 / 32 / 64 / 128 floats that holds the larger one.
// Entries in flight per slot (U): the forward 4, the backward passes 2; half of that at width 128.
template <int PASS, class Args>
void launch_pass(const sextans_engine *e, const Args &a, const int *perm, bool heads_inside, hipStream_t s) {
    constexpr bool F = PASS == sx::kAttnForward, DROP = std::is_same_v<Args, sx::AttnDropArgs>;
    for_width(a.d > a.dv ? a.d : a.dv, [&](auto w) {
        using W = decltype(w);
        launch_pattern<sx::AttnPass<PASS, W::T, W::P, W::k128 ? (F ? 2 : 1) : (F ? 4 : 2), DROP>>(e, a, perm, heads_inside, s);
    });
}

}  // namespace
}  // namespace sxe

using namespace sxe;

namespace {

// both entry points of a pass end here (drop == NULL: the plain one)
int attention_forward(sextans_handle_t h, int heads, int d, int dv, float scale, const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk,
                      const float *d_V, int64_t ldv, const float *d_bias, float *d_O, int64_t ldo, float *d_lse, const sextans_dropout *drop,
                      void *stream) {
    if (int rc = check_dims(h, heads, d, dv)) return rc;   // nothing here needs a device
    const Dropout mode = dropout_mode(drop);
    if (mode == Dropout::kInvalid) return SEXTANS_ERR_INVALID;
    if (mode == Dropout::kPlain) drop = nullptr;
    if (bad_ld(ldq, (int64_t)heads * d) || bad_ld(ldk, (int64_t)heads * d) || bad_ld(ldv, (int64_t)heads * dv) || bad_ld(ldo, (int64_t)heads * dv))
        return SEXTANS_ERR_INVALID;
    if (misaligned(d_Q, d_K, d_V, d_bias, d_O, d_lse)) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    if (int rc = call.open(!d_Q || !d_K || !d_V || !d_O || !d_lse, stream)) return rc;
    if (call.degenerate()) {   // every row is empty
        attention_fill(d_O, h->M, heads * dv, ldo, 0.0f, call.s);
        attention_fill(d_lse, h->M, heads, heads, -INFINITY, call.s);
        return call.done();
    }
    if (int rc = call.tables(false)) return rc;
    sx::AttnArgs a{};
    a.Q = d_Q; a.K = d_K; a.V = d_V; a.bias = d_bias; a.out = d_O; a.out_lse = d_lse;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
    a.H = heads; a.d = d; a.dv = dv; a.scale = scale;
    with_dropout<sx::AttnDropArgs>(a, drop, [&](const auto &args) {
        call.rows([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnForward>(e, args, perm, false, call.s); });
    });
    return call.close("attention_fused", drop != nullptr);
}

int attention_backward(sextans_handle_t h, int heads, int d, int dv, float scale, const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk,
                       const float *d_V, int64_t ldv, const float *d_bias, const float *d_O, int64_t ldo, const float *d_lse, const float *d_G,
                       int64_t ldg, float *d_delta, float *d_dQ, int64_t lddq, float *d_dK, int64_t lddk, float *d_dV, int64_t lddv, float *d_dbias,
                       const sextans_dropout *drop, void *stream) {
    if (int rc = check_dims(h, heads, d, dv)) return rc;
    const Dropout mode = dropout_mode(drop);
    if (mode == Dropout::kInvalid) return SEXTANS_ERR_INVALID;
    if (mode == Dropout::kPlain) drop = nullptr;
    const int64_t hd = (int64_t)heads * d, hdv = (int64_t)heads * dv;
    if (bad_ld(ldq, hd) || bad_ld(ldk, hd) || bad_ld(ldv, hdv) || bad_ld(ldo, hdv) || bad_ld(ldg, hdv) || bad_ld(lddq, hd) || bad_ld(lddk, hd) ||
        bad_ld(lddv, hdv))
        return SEXTANS_ERR_INVALID;
    if (misaligned(d_Q, d_K, d_V, d_bias, d_O, d_lse, d_G, d_delta, d_dQ, d_dK, d_dV, d_dbias)) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    if (int rc = call.open(!d_Q || !d_K || !d_V || !d_O || !d_lse || !d_G || !d_delta || !d_dQ || !d_dK || !d_dV, stream)) return rc;
    if (call.degenerate()) {
        attention_fill(d_delta, h->M, heads, heads, 0.0f, call.s);
        attention_fill(d_dQ, h->M, (int)hd, lddq, 0.0f, call.s);
        attention_fill(d_dK, h->K, (int)hd, lddk, 0.0f, call.s);
        attention_fill(d_dV, h->K, (int)hdv, lddv, 0.0f, call.s);
        return call.done();
    }
    if (int rc = call.tables(true)) return rc;
    sx::AttnArgs a{};
    a.Q = d_Q; a.K = d_K; a.V = d_V; a.bias = d_bias; a.O = d_O; a.lse = d_lse; a.G = d_G; a.delta = d_delta;
    a.out_delta = d_delta; a.dQ = d_dQ; a.dK = d_dK; a.dV = d_dV; a.dbias = d_dbias;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.ldg = ldg; a.lddq = lddq; a.lddk = lddk; a.lddv = lddv;
    a.H = heads; a.d = d; a.dv = dv; a.scale = scale;
    with_dropout<sx::AttnDropArgs>(a, drop, [&](const auto &args) {
        call.rows([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnBackwardRows>(e, args, perm, d_dbias != nullptr, call.s); });
        call.cols([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnBackwardCols>(e, args, perm, false, call.s); });
    });
    return call.close("attention_fused_backward", drop != nullptr);
}

}  // namespace

extern "C" {

int sextans_attention_device(sextans_handle_t h, int heads, int d, int dv, float scale, const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk,
                             const float *d_V, int64_t ldv, const float *d_bias, float *d_O, int64_t ldo, float *d_lse, void *stream) {
    return attention_forward(h, heads, d, dv, scale, d_Q, ldq, d_K, ldk, d_V, ldv, d_bias, d_O, ldo, d_lse, nullptr, stream);
}

int sextans_attention_backward_device(sextans_handle_t h, int heads, int d, int dv, float scale, const float *d_Q, int64_t ldq, const float *d_K,
                                      int64_t ldk, const float *d_V, int64_t ldv, const float *d_bias, const float *d_O, int64_t ldo, const float *d_lse,
                                      const float *d_G, int64_t ldg, float *d_delta, float *d_dQ, int64_t lddq, float *d_dK, int64_t lddk, float *d_dV,
                                      int64_t lddv, float *d_dbias, void *stream) {
    return attention_backward(h, heads, d, dv, scale, d_Q, ldq, d_K, ldk, d_V, ldv, d_bias, d_O, ldo, d_lse, d_G, ldg, d_delta, d_dQ, lddq, d_dK, lddk,
                              d_dV, lddv, d_dbias, nullptr, stream);
}

int sextans_attention_dropout_device(sextans_handle_t h, int heads, int d, int dv, float scale, const float *d_Q, int64_t ldq, const float *d_K,
                                     int64_t ldk, const float *d_V, int64_t ldv, const float *d_bias, float *d_O, int64_t ldo, float *d_lse,
                                     const sextans_dropout *drop, void *stream) {
    return attention_forward(h, heads, d, dv, scale, d_Q, ldq, d_K, ldk, d_V, ldv, d_bias, d_O, ldo, d_lse, drop, stream);
}

int sextans_attention_dropout_backward_device(sextans_handle_t h, int heads, int d, int dv, float scale, const float *d_Q, int64_t ldq, const float *d_K,
                                              int64_t ldk, const float *d_V, int64_t ldv, const float *d_bias, const float *d_O, int64_t ldo,
                                              const float *d_lse, const float *d_G, int64_t ldg, float *d_delta, float *d_dQ, int64_t lddq, float *d_dK,
                                              int64_t lddk, float *d_dV, int64_t lddv, float *d_dbias, const sextans_dropout *drop, void *stream) {
    return attention_backward(h, heads, d, dv, scale, d_Q, ldq, d_K, ldk, d_V, ldv, d_bias, d_O, ldo, d_lse, d_G, ldg, d_delta, d_dQ, lddq, d_dK, lddk,
                              d_dV, lddv, d_dbias, drop, stream);
}

/* nnz * heads multipliers, [e * heads + h]: what the fused dropout kernels recompute, written out (the composition path, tests) */
int sextans_dropout_mask_device(sextans_handle_t h, int heads, const sextans_dropout *drop, float *d_mult, void *stream) {
    if (!h || heads < 1 || !drop || sx::dropout_bad(drop->p, drop->d_step)) return SEXTANS_ERR_INVALID;   // nothing here needs a device
    if (misaligned(d_mult)) return SEXTANS_ERR_INVALID;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    const long long n = (long long)h->nnz * heads;
    if (n == 0) return SEXTANS_OK;
    if (!d_mult) return SEXTANS_ERR_INVALID;
    SX_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(sx::dropout_mask, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       sx::dropout_args(drop->p, drop->seed, drop->d_step), n, d_mult);
    SX_HIP(hipGetLastError());
    h->last_kernel = "dropout_mask";
    return SEXTANS_OK;
}

int sextans_dropout_keep_host(int64_t first, int64_t count, int heads, float p, uint64_t seed, uint64_t step, uint8_t *keep) {
    if (first < 0 || count < 0 || heads < 1 || sx::dropout_bad(p, nullptr) || (count > 0 && !keep)) return SEXTANS_ERR_INVALID;
    const uint64_t key = sx::dropout_key(seed, step);
    const uint32_t thresh = sx::dropout_thresh(p);
    for (int64_t i = 0; i < count; ++i)
        for (int hh = 0; hh < heads; ++hh)
            keep[i * heads + hh] = sx::dropout_u32(key, (uint64_t)(first + i), (uint32_t)heads, (uint32_t)hh) >= thresh ? 1 : 0;
    return SEXTANS_OK;
}

}  // extern "C"
