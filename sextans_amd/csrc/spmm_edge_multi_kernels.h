// spmm_edge_multi_kernels.h -- several aggregations of EDGE-FEATURE messages in one pass over the pattern of a CSR matrix
// (sextans_spmm_edge_multi_device_rm / sextans_spmm_edge_multi_backward_device_rm): the messages of spmm_edge_kernels.h under the
// aggregates of spmm_multi_kernels.h -- PNAConv over an edge MLP's messages (copy), EdgeConv / DGCNN (copy_e_max), u_mul_e_max,
// u_add_e_max.  No counterpart in the reference: its PEs weight an entry with a scalar and only accumulate.
//
//   message        m[e, n] = B[c, n] * E[e, n] | B[c, n] + E[e, n] | relu(B[c, n] + E[e, n]) | E[e, n]   (one rounded fp32 operation:
//                  EdgePass's message, edge_relu included); E[e] is read at (long long)e * lde
//   forward        MOMENTS  sum[r, n] = sum_e m (__fadd_rn);  sumsq[r, n] = sum_e m^2 (s2 = fmaf(m, m, s2))
//                  EXTREMA  max / min[r, n] and argmax / argmin[r, n] by reduce_wins: NaN wins, then the better value, then the smaller
//                           entry position
//                  empty row: sums +0, extrema +0, args -1; a row of one entry: sum has the message's bits, sumsq its rounded square
//   per entry      t[n] = multi_t<GROUPS>(m, e, ..): Gsum, then fmaf(2 m, Gsq, t), then + Gmax where e won, then + Gmin where e won
//   backward cols  (over A^T; E through perm)  dB[c, n] = fmaf(E[e, n], t, dB) | dB + t | dB + (B + E > 0 ? t : 0);  COPY has none
//   backward rows  dE[e, n] = t * B[c, n] | t | (B + E > 0 ? t : +0) | t   (one rounded operation, stored once by the slot that owns
//                  the (entry, tile))
//
// GROUPS is the pair of switches of spmm_multi_kernels.h; the forward's state layout and every combine are MultiPass's own.  The passes
// plug into the row walking of pattern_pass.h as EdgePass does: column tiles in the grid in every pass, a slot of T lanes owns one
// (row, tile).  An operand is loaded only where a formula reads it: compile-time by OP and GROUPS, a uniform branch by which gradients
// are present (m is needed by Gsq alone).  The column pass loads its own B row (B[c]) in begin when Gsq is present or with ADD_RELU.
// No atomics, nothing of size nnz x N beyond E and dE; sums in an order fixed by the pattern and the launch shape, which does not
// depend on GROUPS, on which pointers are NULL or on the entries in flight (a slot adds its entries one after the other).
#pragma once
#include "pattern_pass.h"
#include "spmm_edge_kernels.h"
#include "spmm_multi_kernels.h"

namespace sx {

struct EdgeMultiArgs {
    const float *B, *E;                          // E: (nnz, N) in A's entry order
    float *sum, *sumsq, *mx, *mn;                // forward (each may be null inside its group)
    int *out_argmax, *out_argmin;
    const float *gsum, *gsumsq, *gmax, *gmin;    // backward (each may be null inside its group)
    const int *argmax, *argmin;
    float *dB, *dE;
    long long ldb, lde, ld_sum, ld_sumsq, ld_max, ld_min, ld_arg, lddb, ldde;   // ld_*: of the forward's outputs / the backward's gradients
    int H;                                       // column tiles (the bodies' "heads")
    int N, tile;                                 // tile: floats per tile = 4 T P
};

// the message of one float (b: B[c, n], x: E[e, n]); ADD_RELU: s is the sum before the relu
template <int OP>
__device__ __forceinline__ float edge_message(float b, float x) {
    return OP == kEdgeMul ? __fmul_rn(b, x) : OP == kEdgeAdd ? __fadd_rn(b, x) : OP == kEdgeAddRelu ? edge_relu(__fadd_rn(b, x)) : x;
}

// One slot's view of a pass: the interface of AttnPass.  "own" is the row walked (the column pass: a column of A), ci[e] the other index.
template <int PASS, int OP, int GROUPS, int T_, int P_, int U_>
struct EdgeMultiPass {
    using Args = EdgeMultiArgs;
    using State = MultiPass<PASS, GROUPS, T_, P_, U_>;   // the state layout and the combine
    static constexpr int T = T_, P = P_, U = U_, W = 4 * P_;
    static constexpr bool kMom = State::kMom, kExt = State::kExt;
    static constexpr bool kFwd = PASS == kAttnForward, kRows = PASS == kAttnBackwardRows, kCols = PASS == kAttnBackwardCols;
    static constexpr int kS1 = State::kS1, kS2 = State::kS2, kMax = State::kMax, kMaxPos = State::kMaxPos, kMin = State::kMin,
                         kMinPos = State::kMinPos;
    static constexpr int NF = State::NF;
    static constexpr bool kMerge = State::kMerge;
    static_assert(!(kCols && OP == kEdgeCopy), "COPY has no column pass");
    // what a pass can read at all (the uniform branches below narrow it to what the given gradients need)
    static constexpr bool kOwnB = kCols && (kMom || OP == kEdgeAddRelu);                                       // cols: B[c] of the own column
    static constexpr bool kGatherB = kFwd ? OP != kEdgeCopy : kRows && (OP == kEdgeMul || OP == kEdgeAddRelu || (kMom && OP != kEdgeCopy));
    static constexpr bool kEdge = kFwd || OP == kEdgeAddRelu || kMom || (kCols && OP == kEdgeMul);             // E[e]
    const EdgeMultiArgs &a;
    const int *ci, *perm;
    const int t;
    int h = 0, n = 0;                       // the tile and its valid floats
    float y[kOwnB ? W : 1];                 // cols: the own column's B row
    float gs[kRows && kMom ? W : 1], gq[kRows && kMom ? W : 1];   // rows: the own row's gradients
    float gx[kRows && kExt ? W : 1], gn[kRows && kExt ? W : 1];
    int ax[kRows && kExt ? W : 1], an[kRows && kExt ? W : 1];     // ... and args
    float f[NF];

    __device__ __forceinline__ EdgeMultiPass(const EdgeMultiArgs &a_, const int *ci_, const int *perm_, int t_) : a(a_), ci(ci_), perm(perm_), t(t_) {}

    // m is read by the gradient of sumsq alone
    __device__ __forceinline__ bool needs_m() const { return kMom && a.gsumsq != nullptr; }

    __device__ __forceinline__ void begin(bool act, int own, int tile, bool) {
        h = tile;
        n = min(a.tile, a.N - h * a.tile);
        const long long r = act ? own : 0, c0 = (long long)h * a.tile;
        if (kFwd) {
            if (kMom) {
#pragma unroll
                for (int i = 0; i < 2 * W; ++i) f[i] = 0.0f;
            }
            if (kExt) {
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    f[kMax + i] = -INFINITY;
                    f[kMin + i] = INFINITY;
                    f[kMaxPos + i] = f[kMinPos + i] = __int_as_float(INT_MAX);
                }
            }
        } else if (kRows) {
            if (kMom) {
                attn_load<T, P>(gs, a.gsum + r * a.ld_sum + c0, n, t, act && a.gsum);
                attn_load<T, P>(gq, a.gsumsq + r * a.ld_sumsq + c0, n, t, act && a.gsumsq);
            }
            if (kExt) {
                attn_load<T, P>(gx, a.gmax + r * a.ld_max + c0, n, t, act && a.gmax);
                attn_load<T, P>(gn, a.gmin + r * a.ld_min + c0, n, t, act && a.gmin);
                reduce_load_arg<T, P>(ax, a.argmax + r * a.ld_arg + c0, n, t, act && a.gmax);
                reduce_load_arg<T, P>(an, a.argmin + r * a.ld_arg + c0, n, t, act && a.gmin);
            }
            f[0] = 0.0f;
        } else {
            if (kOwnB) attn_load<T, P>(y, a.B + r * a.ldb + c0, n, t, act && (OP == kEdgeAddRelu || needs_m()));
#pragma unroll
            for (int i = 0; i < NF; ++i) f[i] = 0.0f;
        }
    }

    __device__ __forceinline__ void batch(const int (&e)[U_], const bool (&valid)[U_]) {
        const long long c0 = (long long)h * a.tile;
        long long oth[U];
        int pe[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            oth[u] = ((kGatherB || kCols) && valid[u]) ? ci[e[u]] : 0;
            pe[u] = kCols ? (valid[u] ? perm[e[u]] : 0) : e[u];   // the entry's position in A's arrays
        }
        if (kFwd) {
            float b[U][kGatherB ? W : 1] = {}, x[U][W];   // the gathered B rows and the entries' E rows: issued before the first is used
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (kGatherB) attn_load<T, P>(b[u], a.B + oth[u] * a.ldb + c0, n, t, valid[u]);
                attn_load<T, P>(x[u], a.E + (long long)pe[u] * a.lde + c0, n, t, valid[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!valid[u]) continue;
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const float m = edge_message<OP>(b[u][kGatherB ? i : 0], x[u][i]);
                    if (kMom) {
                        f[kS1 + i] = __fadd_rn(f[kS1 + i], m);
                        f[kS2 + i] = __fmaf_rn(m, m, f[kS2 + i]);
                    }
                    if (kExt) {
                        if (reduce_wins<kReduceMax>(m, pe[u], f[kMax + i], __float_as_int(f[kMaxPos + i]))) {
                            f[kMax + i] = m;
                            f[kMaxPos + i] = __int_as_float(pe[u]);
                        }
                        if (reduce_wins<kReduceMin>(m, pe[u], f[kMin + i], __float_as_int(f[kMinPos + i]))) {
                            f[kMin + i] = m;
                            f[kMinPos + i] = __int_as_float(pe[u]);
                        }
                    }
                }
            }
        } else if (kRows) {
            const bool want_b = OP == kEdgeMul || OP == kEdgeAddRelu || needs_m(), want_e = OP == kEdgeAddRelu || needs_m();
            float b[U][kGatherB ? W : 1] = {}, x[U][kEdge ? W : 1] = {};
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (kGatherB) attn_load<T, P>(b[u], a.B + oth[u] * a.ldb + c0, n, t, valid[u] && want_b);
                if (kEdge) attn_load<T, P>(x[u], a.E + (long long)pe[u] * a.lde + c0, n, t, valid[u] && want_e);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!valid[u]) continue;
                float d[W];
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const float bb = b[u][kGatherB ? i : 0], xx = x[u][kEdge ? i : 0];
                    const float m = kMom ? edge_message<OP>(bb, xx) : 0.0f;
                    const float tt = multi_t<GROUPS>(m, pe[u], a.gsum != nullptr, gs[kMom ? i : 0], a.gsumsq != nullptr, gq[kMom ? i : 0],
                                                     a.gmax != nullptr, ax[kExt ? i : 0], gx[kExt ? i : 0], a.gmin != nullptr,
                                                     an[kExt ? i : 0], gn[kExt ? i : 0]);
                    d[i] = OP == kEdgeMul ? __fmul_rn(tt, bb) : OP == kEdgeAddRelu ? (__fadd_rn(bb, xx) > 0.0f ? tt : 0.0f) : tt;
                }
                attn_store<T, P>(d, a.dE + (long long)pe[u] * a.ldde + c0, n, t);
            }
        } else {
            // the column pass: the gradients and args of the entries' rows, and the entries' E rows through perm
            const bool want_e = OP == kEdgeMul || OP == kEdgeAddRelu || needs_m();
            float qs[U][kMom ? W : 1], qq[U][kMom ? W : 1], qx[U][kExt ? W : 1], qn[U][kExt ? W : 1], x[U][kEdge ? W : 1] = {};
            int ix[U][kExt ? W : 1], im[U][kExt ? W : 1];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (kMom) {
                    attn_load<T, P>(qs[u], a.gsum + oth[u] * a.ld_sum + c0, n, t, valid[u] && a.gsum);
                    attn_load<T, P>(qq[u], a.gsumsq + oth[u] * a.ld_sumsq + c0, n, t, valid[u] && a.gsumsq);
                }
                if (kExt) {
                    reduce_load_arg<T, P>(ix[u], a.argmax + oth[u] * a.ld_arg + c0, n, t, valid[u] && a.gmax);
                    attn_load<T, P>(qx[u], a.gmax + oth[u] * a.ld_max + c0, n, t, valid[u] && a.gmax);
                    reduce_load_arg<T, P>(im[u], a.argmin + oth[u] * a.ld_arg + c0, n, t, valid[u] && a.gmin);
                    attn_load<T, P>(qn[u], a.gmin + oth[u] * a.ld_min + c0, n, t, valid[u] && a.gmin);
                }
                if (kEdge) attn_load<T, P>(x[u], a.E + (long long)pe[u] * a.lde + c0, n, t, valid[u] && want_e);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!valid[u]) continue;
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const float bb = y[kOwnB ? i : 0], xx = x[u][kEdge ? i : 0];
                    const float m = kMom ? edge_message<OP>(bb, xx) : 0.0f;
                    const float tt = multi_t<GROUPS>(m, pe[u], a.gsum != nullptr, qs[u][kMom ? i : 0], a.gsumsq != nullptr, qq[u][kMom ? i : 0],
                                                     a.gmax != nullptr, ix[u][kExt ? i : 0], qx[u][kExt ? i : 0], a.gmin != nullptr,
                                                     im[u][kExt ? i : 0], qn[u][kExt ? i : 0]);
                    if (OP == kEdgeMul) f[i] = __fmaf_rn(xx, tt, f[i]);
                    else if (OP == kEdgeAdd) f[i] = __fadd_rn(f[i], tt);
                    else f[i] = __fadd_rn(f[i], __fadd_rn(bb, xx) > 0.0f ? tt : 0.0f);
                }
            }
        }
    }

    static __device__ __forceinline__ void combine(float *g, const float *o) { State::combine(g, o); }

    // a position still at INT_MAX: the row has no entry -- (+0, -1)
    __device__ __forceinline__ void finish(bool writer, int own, int) {
        if (!writer || kRows) return;
        const long long r = own, c0 = (long long)h * a.tile;
        if (kFwd) {
            if (kMom) {
                if (a.sum) attn_store<T, P>(f + kS1, a.sum + r * a.ld_sum + c0, n, t);
                if (a.sumsq) attn_store<T, P>(f + kS2, a.sumsq + r * a.ld_sumsq + c0, n, t);
            }
            if (kExt) {
                float c[W];
                int g[W];
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const int idx = __float_as_int(f[kMaxPos + i]);
                    c[i] = idx == INT_MAX ? 0.0f : f[kMax + i];
                    g[i] = idx == INT_MAX ? -1 : idx;
                }
                if (a.mx) attn_store<T, P>(c, a.mx + r * a.ld_max + c0, n, t);
                if (a.out_argmax) multi_store_arg<T, P>(g, a.out_argmax + r * a.ld_arg + c0, n, t);
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const int idx = __float_as_int(f[kMinPos + i]);
                    c[i] = idx == INT_MAX ? 0.0f : f[kMin + i];
                    g[i] = idx == INT_MAX ? -1 : idx;
                }
                if (a.mn) attn_store<T, P>(c, a.mn + r * a.ld_min + c0, n, t);
                if (a.out_argmin) multi_store_arg<T, P>(g, a.out_argmin + r * a.ld_arg + c0, n, t);
            }
        } else {
            attn_store<T, P>(f, a.dB + r * a.lddb + c0, n, t);
        }
    }
};

}  // namespace sx
