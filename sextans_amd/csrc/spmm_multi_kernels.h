// spmm_multi_kernels.h -- several aggregations of the same messages in one pass over a CSR matrix (sextans_spmm_multi_device_rm /
// sextans_spmm_multi_backward_device_rm): the sum, the sum of squares, the max and the min (with their args) that PNA, PyG's
// MultiAggregation and the mean || max read-outs take of a node's neighbours.  No counterpart in the reference: its PEs only multiply
// and accumulate.
//
//   message        p_e[n] = val[e] * B[c, n]  (one rounded fp32 product, __fmul_rn: the message of spmm_reduce_kernels.h)
//   forward        MOMENTS  sum[r, n] = sum_e p_e (__fadd_rn);  sumsq[r, n] = sum_e p_e^2 (s2 = fmaf(p, p, s2))
//                  EXTREMA  max / min[r, n] and argmax / argmin[r, n]: reduce_wins<OP> of spmm_reduce_kernels.h itself -- NaN beats every
//                           number, then the better product, then the smaller position; the bits of sextans_spmm_reduce_device_rm
//                  empty row: sums +0, max and min +0, args -1
//   per entry      t[n] = Gsum[r, n] + 2 p_e[n] Gsq[r, n] + (argmax[r, n] == e ? Gmax[r, n] : 0) + (argmin[r, n] == e ? Gmin[r, n] : 0)
//                  over the gradients that are present, IN THIS ORDER (multi_t below):
//                      t = Gsum (0 without it);  t = fmaf(2 p, Gsq, t)  (2 p is exact);  t = t + Gmax where the entry won;  t = t + Gmin
//   backward cols  (over A^T)  dB[c, n] = sum over the entries of column c of val[e] * t[n]      (dB = fmaf(val_e, t, dB))
//   backward rows  dval[e] = sum_n B[c, n] * t[n]                                                (fmaf over the pieces, a butterfly)
//
// GROUPS is a compile-time pair of switches (kMultiMoments, kMultiExtrema): three variants.  Inside a computed group an output or a
// gradient whose pointer is NULL is not stored / not read (a uniform branch).
// The passes plug into the row walking of pattern_pass.h exactly as ReducePass does; COLUMN TILES play the heads' part: a slot of T
// lanes owns one (row, tile), lane t holds the 16-byte pieces t, t + T, .. of the tile, the last tile may be partial.  One gathered B row
// per entry serves every aggregate.  The forward's state per float is s1, s2, (best, position) for max and for min -- 6 W floats at
// most; combine adds the sums and merges the extrema lexicographically (ReducePass::combine's comparison).  The column pass loads its
// own B row (B[c]) in begin when the MOMENTS group is on (p_e needs it); the row pass ("tiles inside") keeps the own row's gradients
// and args of the tile, and one lane owns dval[e] for every tile and adds the tiles in ascending order.
// No atomics; the sums run in an order fixed by the pattern and the launch shape: the same bits on every run.  The sums' order does
// not depend on GROUPS or on which pointers are NULL: each group alone gives the bits of the full call.
#pragma once
#include "pattern_pass.h"
#include "spmm_reduce_kernels.h"

namespace sx {

enum { kMultiMoments = 1, kMultiExtrema = 2 };

struct MultiArgs {
    const float *val, *B;                        // val: nnz floats in A's entry order
    float *sum, *sumsq, *mx, *mn;                // forward (each may be null inside its group)
    int *out_argmax, *out_argmin;
    const float *gsum, *gsumsq, *gmax, *gmin;    // backward (each may be null inside its group)
    const int *argmax, *argmin;
    float *dB, *dval;
    long long ldb, ld_sum, ld_sumsq, ld_max, ld_min, ld_arg, lddb;   // ld_*: of the forward's outputs / the backward's gradients
    int H;                                       // column tiles (the bodies' "heads")
    int N, tile;                                 // tile: floats per tile = 4 T P
};

template <int T, int P>
__device__ __forceinline__ void multi_store_arg(const int *g, int *row, int n, int t) {
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int col = 4 * (t + T * k);
        if (col < n) *reinterpret_cast<int4 *>(row + col) = make_int4(g[4 * k], g[4 * k + 1], g[4 * k + 2], g[4 * k + 3]);
    }
}

// t of one float (the order of the adds is part of the contract: see above); has_*: the gradient is present
template <int GROUPS>
__device__ __forceinline__ float multi_t(float p, int pe, bool has_sum, float gs, bool has_sq, float gq, bool has_max, int amax, float gx,
                                         bool has_min, int amin, float gn) {
    float t = 0.0f;
    if (GROUPS & kMultiMoments) {
        if (has_sum) t = gs;
        if (has_sq) t = __fmaf_rn(__fadd_rn(p, p), gq, t);
    }
    if (GROUPS & kMultiExtrema) {
        if (has_max && amax == pe) t = __fadd_rn(t, gx);
        if (has_min && amin == pe) t = __fadd_rn(t, gn);
    }
    return t;
}

// One slot's view of a pass: the interface of AttnPass.  "own" is the row walked (the column pass: a column of A), ci[e] the other index.
template <int PASS, int GROUPS, int T_, int P_, int U_>
struct MultiPass {
    using Args = MultiArgs;
    static constexpr int T = T_, P = P_, U = U_, W = 4 * P_;
    static constexpr bool kMom = (GROUPS & kMultiMoments) != 0, kExt = (GROUPS & kMultiExtrema) != 0;
    // forward: s1, s2 | max best, max position, min best, min position; rows: nothing to merge; cols: dB
    static constexpr int kS1 = 0, kS2 = W, kMax = kMom ? 2 * W : 0, kMaxPos = kMax + W, kMin = kMax + 2 * W, kMinPos = kMax + 3 * W;
    static constexpr int NF = PASS == kAttnForward ? (kMom ? 2 * W : 0) + (kExt ? 4 * W : 0) : PASS == kAttnBackwardRows ? 1 : W;
    static constexpr bool kMerge = PASS != kAttnBackwardRows;
    const MultiArgs &a;
    const int *ci, *perm;
    const int t;
    int h = 0, n = 0;                                   // the tile and its valid floats
    float y[PASS == kAttnBackwardCols && kMom ? W : 1]; // cols: the own column's B row
    float gs[PASS == kAttnBackwardRows && kMom ? W : 1], gq[PASS == kAttnBackwardRows && kMom ? W : 1];   // rows: the own row's gradients
    float gx[PASS == kAttnBackwardRows && kExt ? W : 1], gn[PASS == kAttnBackwardRows && kExt ? W : 1];
    int ax[PASS == kAttnBackwardRows && kExt ? W : 1], an[PASS == kAttnBackwardRows && kExt ? W : 1];     // ... and args
    float f[NF];

    __device__ __forceinline__ MultiPass(const MultiArgs &a_, const int *ci_, const int *perm_, int t_) : a(a_), ci(ci_), perm(perm_), t(t_) {}

    __device__ __forceinline__ void begin(bool act, int own, int tile, bool) {
        h = tile;
        n = min(a.tile, a.N - h * a.tile);
        const long long r = act ? own : 0, c0 = (long long)h * a.tile;
        if (PASS == kAttnForward) {
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
        } else if (PASS == kAttnBackwardRows) {
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
            if (kMom) attn_load<T, P>(y, a.B + r * a.ldb + c0, n, t, act && a.gsumsq);
#pragma unroll
            for (int i = 0; i < NF; ++i) f[i] = 0.0f;
        }
    }

    __device__ __forceinline__ void batch(const int (&e)[U_], const bool (&valid)[U_]) {
        constexpr bool kCols = PASS == kAttnBackwardCols;
        const long long c0 = (long long)h * a.tile;
        long long oth[U];
        int pe[U];
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            oth[u] = valid[u] ? ci[e[u]] : 0;
            pe[u] = kCols ? (valid[u] ? perm[e[u]] : 0) : e[u];   // the entry's position in A's arrays
        }
        if (!kCols) {
            float b[U][W];   // the gathered B rows: issued before the first is used
#pragma unroll
            for (int u = 0; u < U; ++u) {
                attn_load<T, P>(b[u], a.B + oth[u] * a.ldb + c0, n, t, valid[u]);
                v[u] = valid[u] ? a.val[pe[u]] : 0.0f;
            }
            if (PASS == kAttnForward) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (!valid[u]) continue;
#pragma unroll
                    for (int i = 0; i < W; ++i) {
                        const float p = __fmul_rn(v[u], b[u][i]);
                        if (kMom) {
                            f[kS1 + i] = __fadd_rn(f[kS1 + i], p);
                            f[kS2 + i] = __fmaf_rn(p, p, f[kS2 + i]);
                        }
                        if (kExt) {
                            if (reduce_wins<kReduceMax>(p, pe[u], f[kMax + i], __float_as_int(f[kMaxPos + i]))) {
                                f[kMax + i] = p;
                                f[kMaxPos + i] = __int_as_float(pe[u]);
                            }
                            if (reduce_wins<kReduceMin>(p, pe[u], f[kMin + i], __float_as_int(f[kMinPos + i]))) {
                                f[kMin + i] = p;
                                f[kMinPos + i] = __int_as_float(pe[u]);
                            }
                        }
                    }
                }
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    float s = 0.0f;
#pragma unroll
                    for (int i = 0; i < W; ++i) {
                        const float p = __fmul_rn(v[u], b[u][i]);
                        const float tt = multi_t<GROUPS>(p, pe[u], a.gsum != nullptr, gs[kMom ? i : 0], a.gsumsq != nullptr, gq[kMom ? i : 0],
                                                         a.gmax != nullptr, ax[kExt ? i : 0], gx[kExt ? i : 0], a.gmin != nullptr,
                                                         an[kExt ? i : 0], gn[kExt ? i : 0]);
                        s = __fmaf_rn(b[u][i], tt, s);
                    }
                    s = group_sum<T>(s);
                    // the tiles of an entry are taken by this lane one after the other, in ascending order: a plain read-modify-write
                    if (valid[u] && t == 0) a.dval[pe[u]] = h == 0 ? s : __fadd_rn(a.dval[pe[u]], s);
                }
            }
        } else {
            // the column pass: the gradients and args of the entries' rows
            float qs[U][kMom ? W : 1], qq[U][kMom ? W : 1], qx[U][kExt ? W : 1], qn[U][kExt ? W : 1];
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
                v[u] = valid[u] ? a.val[pe[u]] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!valid[u]) continue;
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const float p = kMom ? __fmul_rn(v[u], y[kMom ? i : 0]) : 0.0f;
                    const float tt = multi_t<GROUPS>(p, pe[u], a.gsum != nullptr, qs[u][kMom ? i : 0], a.gsumsq != nullptr, qq[u][kMom ? i : 0],
                                                     a.gmax != nullptr, ix[u][kExt ? i : 0], qx[u][kExt ? i : 0], a.gmin != nullptr,
                                                     im[u][kExt ? i : 0], qn[u][kExt ? i : 0]);
                    f[i] = __fmaf_rn(v[u], tt, f[i]);
                }
            }
        }
    }

    // g <- g (+) o: both sides of a butterfly exchange end with the same bits (the adds commute; the comparison is a total order on
    // distinct positions)
    static __device__ __forceinline__ void combine(float *g, const float *o) {
        if (PASS == kAttnForward) {
            if (kMom) {
#pragma unroll
                for (int i = 0; i < 2 * W; ++i) g[i] = __fadd_rn(g[i], o[i]);
            }
            if (kExt) {
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    if (reduce_wins<kReduceMax>(o[kMax + i], __float_as_int(o[kMaxPos + i]), g[kMax + i], __float_as_int(g[kMaxPos + i]))) {
                        g[kMax + i] = o[kMax + i];
                        g[kMaxPos + i] = o[kMaxPos + i];
                    }
                    if (reduce_wins<kReduceMin>(o[kMin + i], __float_as_int(o[kMinPos + i]), g[kMin + i], __float_as_int(g[kMinPos + i]))) {
                        g[kMin + i] = o[kMin + i];
                        g[kMinPos + i] = o[kMinPos + i];
                    }
                }
            }
        } else if (PASS == kAttnBackwardCols) {
#pragma unroll
            for (int i = 0; i < NF; ++i) g[i] = __fadd_rn(g[i], o[i]);
        }
    }

    // a position still at INT_MAX: the row has no entry -- (+0, -1)
    __device__ __forceinline__ void finish(bool writer, int own, int) {
        if (!writer || PASS == kAttnBackwardRows) return;
        const long long r = own, c0 = (long long)h * a.tile;
        if (PASS == kAttnForward) {
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
