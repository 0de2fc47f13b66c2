// engine_gatv2.hip -- fused GATv2 graph attention over the pattern of the CSR matrix on an engine handle (include/sextans_amd.h):
//   sextans_gatv2_workspace_floats            the floats of workspace the backward needs (datt_rows, then the chunk sums)
//   sextans_gatv2_attention_device            O = softmax(att . LeakyReLU(x_dst[r] + x_src[c]) + bias on A's pattern) x_src per head, and lse
//   sextans_gatv2_attention_backward_device   dx_dst, dx_src, datt (and dbias): a row pass over A, a column pass over A^T, the two-level datt sum
//   sextans_gatv2_attention_dropout_device / _dropout_backward_device   the same with dropout on the attention coefficients (dropout_hash.h)
// Kernels: gatv2_kernels.h on the row walking of pattern_pass.h; the entry points' frame: pattern_launch.h.  A's values are never read.
#include "gatv2_kernels.h"
#include "pattern_launch.h"

namespace sxe {
namespace {

// e: the engine whose CSR arrays and softmax tables the pass walks (the column pass: the companion).  The slot width follows d alone:
// the smallest of 8 / 16 / 32 / 64 / 128 floats that holds it.  Entries in flight per slot (U): the forward takes the GAT forward's 4
// (2 at width 128); the backward passes start from the dot-product kernels' backward 2 (1 at width 128), since they hold as many rows
// (rows: own x_dst, att, G and two accumulators; cols: two gathered rows per entry).  The backward U is UNTUNED: no other value has been
// timed.  No instantiation uses scratch (profiles/gatv2_kernel_resources.txt).
// COUPLING with GatPass (tests/test_gatv2_attention_gpu.py, att = e_0): with att[h, :] = (1, 0, .., 0) and no bias the score is
// LeakyReLU(x_dst[r,h,0] + x_src[c,h,0]), and O and lse are compared BIT FOR BIT with gat_attention on those scalars and V = x_src.  That
// holds only while both forwards form the same batches -- the same T, P and U per width as engine_gat.hip's forward -- and make the
// same roundings after the score.  Retune either forward's U or the walk's order and that comparison has to be looked at again.
template <int PASS, class Args>
void launch_pass(const sextans_engine *e, const Args &a, const int *perm, bool heads_inside, hipStream_t s) {
    constexpr bool F = PASS == sx::kAttnForward, DROP = std::is_same_v<Args, sx::Gatv2DropArgs>;
    for_width(a.d, [&](auto w) {
        using W = decltype(w);
        launch_pattern<sx::Gatv2Pass<PASS, W::T, W::P, W::k128 ? (F ? 2 : 1) : (F ? 4 : 2), DROP>>(e, a, perm, heads_inside, s);
    });
}

static_assert(sx::kGatv2Chunk == 256, "chunks_of (pattern_launch.h) counts the chunks of gatv2_datt_chunks");

}  // namespace

// (engine_state.h) the datt sum; engine_softagg.hip's dt goes through it too
void column_sum_two_level(const float *rows, int64_t M, int hd, float *part, float *out, hipStream_t s) {
    const int64_t nchunks = chunks_of(M);
    hipLaunchKernelGGL(sx::gatv2_datt_chunks, dim3((unsigned)nchunks), dim3(256), 0, s, rows, (long long)M, hd, part);
    hipLaunchKernelGGL(sx::gatv2_datt_total, dim3((unsigned)((hd + 255) / 256)), dim3(256), 0, s, part, (long long)nchunks, hd, out);
}

}  // namespace sxe

using namespace sxe;

extern "C" {

int64_t sextans_gatv2_workspace_floats(sextans_handle_t h, int heads, int d) {
    if (!h || heads < 1 || bad_dim(d)) return -(int64_t)SEXTANS_ERR_INVALID;
    if (!h->d_rp) return -(int64_t)SEXTANS_ERR_STATE;
    const int64_t hd = (int64_t)heads * d;
    return (int64_t)h->M * hd + chunks_of(h->M) * hd;
}

}  // extern "C"

namespace {

// both entry points of a pass end here (drop == NULL: the plain one)
int gatv2_forward(sextans_handle_t h, int heads, int d, float negative_slope, const float *d_xdst, int64_t ldxd, const float *d_xsrc, int64_t ldxs,
                  const float *d_att, const float *d_bias, float *d_O, int64_t ldo, float *d_lse, const sextans_dropout *drop, void *stream) {
    if (!h || heads < 1 || bad_dim(d) || bad_slope(negative_slope)) return SEXTANS_ERR_INVALID;   // nothing here needs a device
    const Dropout mode = dropout_mode(drop);
    if (mode == Dropout::kInvalid) return SEXTANS_ERR_INVALID;
    if (mode == Dropout::kPlain) drop = nullptr;
    const int64_t hd = (int64_t)heads * d;
    if (bad_ld(ldxd, hd) || bad_ld(ldxs, hd) || bad_ld(ldo, hd)) return SEXTANS_ERR_INVALID;
    if (misaligned(d_xdst, d_xsrc, d_att, d_bias, d_O, d_lse)) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    if (int rc = call.open(!d_xdst || !d_xsrc || !d_att || !d_O || !d_lse, stream)) return rc;
    if (call.degenerate()) {   // every row is empty
        attention_fill(d_O, h->M, (int)hd, ldo, 0.0f, call.s);
        attention_fill(d_lse, h->M, heads, heads, -INFINITY, call.s);
        return call.done();
    }
    if (int rc = call.tables(false)) return rc;
    sx::Gatv2Args a{};
    a.xdst = d_xdst; a.xsrc = d_xsrc; a.att = d_att; a.bias = d_bias; a.out = d_O; a.out_lse = d_lse;
    a.ldxd = ldxd; a.ldxs = ldxs; a.ldo = ldo;
    a.H = heads; a.d = d; a.slope = negative_slope;
    with_dropout<sx::Gatv2DropArgs>(a, drop, [&](const auto &args) {
        call.rows([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnForward>(e, args, perm, false, call.s); });
    });
    return call.close("gatv2_fused", drop != nullptr);
}

int gatv2_backward(sextans_handle_t h, int heads, int d, float negative_slope, const float *d_xdst, int64_t ldxd, const float *d_xsrc, int64_t ldxs,
                   const float *d_att, const float *d_bias, const float *d_O, int64_t ldo, const float *d_lse, const float *d_G, int64_t ldg,
                   float *d_delta, float *d_dxdst, int64_t lddxd, float *d_dxsrc, int64_t lddxs, float *d_datt, float *d_work, float *d_dbias,
                   const sextans_dropout *drop, void *stream) {
    if (!h || heads < 1 || bad_dim(d) || bad_slope(negative_slope)) return SEXTANS_ERR_INVALID;
    const Dropout mode = dropout_mode(drop);
    if (mode == Dropout::kInvalid) return SEXTANS_ERR_INVALID;
    if (mode == Dropout::kPlain) drop = nullptr;
    const int64_t hd = (int64_t)heads * d;
    if (bad_ld(ldxd, hd) || bad_ld(ldxs, hd) || bad_ld(ldo, hd) || bad_ld(ldg, hd) || bad_ld(lddxd, hd) || bad_ld(lddxs, hd)) return SEXTANS_ERR_INVALID;
    if (misaligned(d_xdst, d_xsrc, d_att, d_bias, d_O, d_lse, d_G, d_delta, d_dxdst, d_dxsrc, d_datt, d_work, d_dbias)) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    if (int rc = call.open(!d_xdst || !d_xsrc || !d_att || !d_O || !d_lse || !d_G || !d_delta || !d_dxdst || !d_dxsrc || !d_datt || !d_work, stream))
        return rc;
    float *d_part = d_work ? d_work + (int64_t)h->M * hd : nullptr;
    if (call.degenerate()) {
        attention_fill(d_delta, h->M, heads, heads, 0.0f, call.s);
        attention_fill(d_dxdst, h->M, (int)hd, lddxd, 0.0f, call.s);
        attention_fill(d_dxsrc, h->K, (int)hd, lddxs, 0.0f, call.s);
        attention_fill(d_work, h->M, (int)hd, hd, 0.0f, call.s);   // datt_rows and the chunk sums: what the passes would have left
        attention_fill(d_part, chunks_of(h->M), (int)hd, hd, 0.0f, call.s);
        attention_fill(d_datt, 1, (int)hd, hd, 0.0f, call.s);
        return call.done();
    }
    if (int rc = call.tables(true)) return rc;
    sx::Gatv2Args a{};
    a.xdst = d_xdst; a.xsrc = d_xsrc; a.att = d_att; a.bias = d_bias; a.O = d_O; a.lse = d_lse; a.G = d_G; a.delta = d_delta;
    a.out_delta = d_delta; a.dxdst = d_dxdst; a.dxsrc = d_dxsrc; a.datt_rows = d_work; a.dbias = d_dbias;
    a.ldxd = ldxd; a.ldxs = ldxs; a.ldo = ldo; a.ldg = ldg; a.lddxd = lddxd; a.lddxs = lddxs;
    a.H = heads; a.d = d; a.slope = negative_slope;
    with_dropout<sx::Gatv2DropArgs>(a, drop, [&](const auto &args) {
        call.rows([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnBackwardRows>(e, args, perm, d_dbias != nullptr, call.s); });
        call.cols([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnBackwardCols>(e, args, perm, false, call.s); });
    });
    column_sum_two_level(d_work, h->M, (int)hd, d_part, d_datt, call.s);
    return call.close("gatv2_fused_backward", drop != nullptr);
}

}  // namespace

extern "C" {

int sextans_gatv2_attention_device(sextans_handle_t h, int heads, int d, float negative_slope, const float *d_xdst, int64_t ldxd, const float *d_xsrc,
                                   int64_t ldxs, const float *d_att, const float *d_bias, float *d_O, int64_t ldo, float *d_lse, void *stream) {
    return gatv2_forward(h, heads, d, negative_slope, d_xdst, ldxd, d_xsrc, ldxs, d_att, d_bias, d_O, ldo, d_lse, nullptr, stream);
}

int sextans_gatv2_attention_backward_device(sextans_handle_t h, int heads, int d, float negative_slope, const float *d_xdst, int64_t ldxd,
                                            const float *d_xsrc, int64_t ldxs, const float *d_att, const float *d_bias, const float *d_O, int64_t ldo,
                                            const float *d_lse, const float *d_G, int64_t ldg, float *d_delta, float *d_dxdst, int64_t lddxd,
                                            float *d_dxsrc, int64_t lddxs, float *d_datt, float *d_work, float *d_dbias, void *stream) {
    return gatv2_backward(h, heads, d, negative_slope, d_xdst, ldxd, d_xsrc, ldxs, d_att, d_bias, d_O, ldo, d_lse, d_G, ldg, d_delta, d_dxdst, lddxd,
                          d_dxsrc, lddxs, d_datt, d_work, d_dbias, nullptr, stream);
}

int sextans_gatv2_attention_dropout_device(sextans_handle_t h, int heads, int d, float negative_slope, const float *d_xdst, int64_t ldxd,
                                           const float *d_xsrc, int64_t ldxs, const float *d_att, const float *d_bias, float *d_O, int64_t ldo,
                                           float *d_lse, const sextans_dropout *drop, void *stream) {
    return gatv2_forward(h, heads, d, negative_slope, d_xdst, ldxd, d_xsrc, ldxs, d_att, d_bias, d_O, ldo, d_lse, drop, stream);
}

int sextans_gatv2_attention_dropout_backward_device(sextans_handle_t h, int heads, int d, float negative_slope, const float *d_xdst, int64_t ldxd,
                                                    const float *d_xsrc, int64_t ldxs, const float *d_att, const float *d_bias, const float *d_O,
                                                    int64_t ldo, const float *d_lse, const float *d_G, int64_t ldg, float *d_delta, float *d_dxdst,
                                                    int64_t lddxd, float *d_dxsrc, int64_t lddxs, float *d_datt, float *d_work, float *d_dbias,
                                                    const sextans_dropout *drop, void *stream) {
    return gatv2_backward(h, heads, d, negative_slope, d_xdst, ldxd, d_xsrc, ldxs, d_att, d_bias, d_O, ldo, d_lse, d_G, ldg, d_delta, d_dxdst, lddxd,
                          d_dxsrc, lddxs, d_datt, d_work, d_dbias, drop, stream);
}

}  // extern "C"
