// spmm_edge_softagg_kernels.h -- softmax aggregation of EDGE-FEATURE messages over a CSR pattern (sextans_spmm_edge_softagg_device_rm /
// sextans_spmm_edge_softagg_backward_device_rm): GENConv / DeeperGCN on graphs with edge features (message relu(x_j + e_ij) + eps), PyG's
// SoftmaxAggregation over any materialised message.  The messages of spmm_edge_kernels.h under the softmax of spmm_softagg_kernels.h.
// No counterpart in the reference.
//
//   m_e = B[c, n] * E[e, n] | B[c, n] + E[e, n] | edge_relu(B[c, n] + E[e, n]) | E[e, n]     ONE rounded fp32 operation, spmm_edge's
//   s_e = t[n] * m_e   (t == NULL: s_e = m_e)                                                ONE rounded multiply, never fused
//   forward        lse[r, n] = log sum_e exp(s_e);  w_e = exp(s_e - lse[r, n]);  C[r, n] = sum_e w_e m_e.  Empty row: C = +0, lse = -inf
//   backward, G the upstream gradient, q_e = (G[r, n] w_e) fma(t[n], m_e - C[r, n], 1)   (= dL/dm_e):
//     rows             dE[e, n] = q_e B[c, n] (MUL) | q_e (ADD, COPY) | (B + E > 0 ? q_e : +0) (ADD_RELU), stored once per (entry, tile)
//                      dt_rows[r, n] = G[r, n] sum_e w_e m_e (m_e - C[r, n]);  dt[n] = sum_r dt_rows[r, n]  (the two-level sum of GATv2's datt)
//     cols (over A^T)  dB[c, n] = sum over the entries of column c of fma(q_e, E[e, n], .) (MUL) | q_e (ADD) | (B + E > 0 ? q_e : 0) (ADD_RELU);
//                      COPY has none
//
// Only A's PATTERN is read; E and dE are (nnz, N) row-major in A's entry order, addressed as (long long)e * ld.  The passes plug into the
// row walking of pattern_pass.h as SoftaggPass and EdgePass do: COLUMN TILES of at most 64 floats play the heads' part, a slot of T lanes
// owns one (row, tile), the last tile of a row may be partial.  All three passes compute m_e and s_e with the same two functions
// (edge_message, score): they see the same bits.
// The forward is SoftaggPass's online softmax with another source of the message: the state (m, z, acc) per float, the same batch and
// combine arithmetic, __fdiv_rn and softagg_log in finish -- with E[e, :] = val[e] and MUL it returns spmm_softagg's bits.
// The row pass does NOT take the tiles inside the slot (there is no dval to add up over tiles): every (entry, tile) piece of dE is stored
// by the slot that owns it, as in EdgePass; its state is the tile's dt sum (W floats, merged by adds), kept whether or not dt is asked
// for and stored when dt_rows is given; the dE store is predicated on its pointer (engine_edge_softagg.hip says why).
// No atomics; sums in an order fixed by the pattern and the launch shape.
#pragma once
#include "spmm_edge_kernels.h"
#include "spmm_softagg_kernels.h"

namespace sx {

struct EdgeSoftaggArgs {
    const float *B, *E, *t;     // t: N floats or null (= 1)
    const float *C, *lse, *G;   // backward
    float *out, *out_lse;       // forward; out_lse may be null
    float *dB, *dE, *dt_rows;   // backward, each may be null; dt_rows: M x N floats, leading dimension N
    long long ldb, lde, ldc, ldlse, ldg, lddb, ldde;
    int H;                      // column tiles (the bodies' "heads")
    int N, tile;                // tile: floats per tile = 4 T P
};

// the message of spmm_edge_kernels.h: one rounded operation (b is not read for COPY)
template <int OP>
__device__ __forceinline__ float edge_message(float b, float x) {
    return OP == kEdgeMul ? __fmul_rn(b, x) : OP == kEdgeAdd ? __fadd_rn(b, x) : OP == kEdgeAddRelu ? edge_relu(__fadd_rn(b, x)) : x;
}

// One slot's view of a pass: the interface of AttnPass.  "own" is the row walked (the column pass: a column of A), ci[e] the other index.
template <int PASS, int OP, int T_, int P_, int U_>
struct EdgeSoftaggPass {
    using Args = EdgeSoftaggArgs;
    static constexpr int T = T_, P = P_, U = U_, W = 4 * P_;
    static constexpr int NF = PASS == kAttnForward ? 3 * W : W;   // forward: m, z, acc per float; rows: the dt sum; cols: dB
    static constexpr bool kMerge = true;
    static constexpr bool kB = OP != kEdgeCopy;   // the message reads B
    const EdgeSoftaggArgs &a;
    const int *ci, *perm;
    const int t;
    int h = 0, n = 0;        // the tile and its valid floats
    float tt[W];             // the tile's temperatures
    float x[W], y[W], z[W];  // backward: the own column's B (cols) or the own row's C (rows); rows: the own row's lse and G
    float f[NF];

    __device__ __forceinline__ EdgeSoftaggPass(const EdgeSoftaggArgs &a_, const int *ci_, const int *perm_, int t_)
        : a(a_), ci(ci_), perm(perm_), t(t_) {}

    __device__ __forceinline__ void begin(bool act, int own, int tile, bool) {
        h = tile;
        n = min(a.tile, a.N - h * a.tile);
        const long long r = act ? own : 0, c0 = (long long)h * a.tile;
        if (a.t) {
            attn_load<T, P>(tt, a.t + c0, n, t, true);
        } else {
#pragma unroll
            for (int i = 0; i < W; ++i) tt[i] = 1.0f;
        }
        if (PASS == kAttnForward) {
#pragma unroll
            for (int i = 0; i < W; ++i) {
                f[i] = -INFINITY;
                f[W + i] = 0.0f;
                f[2 * W + i] = 0.0f;
            }
        } else {
            if (PASS == kAttnBackwardRows) {
                attn_load<T, P>(x, a.C + r * a.ldc + c0, n, t, act);
                attn_load<T, P>(y, a.lse + r * a.ldlse + c0, n, t, act);
                attn_load<T, P>(z, a.G + r * a.ldg + c0, n, t, act);
            } else {
                attn_load<T, P>(x, a.B + r * a.ldb + c0, n, t, act);
            }
#pragma unroll
            for (int i = 0; i < NF; ++i) f[i] = 0.0f;
        }
    }

    __device__ __forceinline__ float score(float m, int i) const { return a.t ? __fmul_rn(tt[i], m) : m; }
    // q_e from the row's C, lse and G at this float: w = exp(s - lse), gw = G w, d = m - C, q = gw fma(t, d, 1)
    __device__ __forceinline__ float grad(float m, float c, float l, float g, int i, float &gw, float &d) const {
        const float w = softmax_exp(__fsub_rn(score(m, i), l));
        d = __fsub_rn(m, c);
        gw = __fmul_rn(g, w);
        return a.t ? __fmul_rn(gw, __fmaf_rn(tt[i], d, 1.0f)) : __fmul_rn(gw, __fadd_rn(d, 1.0f));
    }

    __device__ __forceinline__ void batch(const int (&e)[U_], const bool (&valid)[U_]) {
        constexpr bool COLS = PASS == kAttnBackwardCols;
        constexpr bool kGather = !COLS && kB;   // forward, rows: the entry's B row
        long long oth[U], pe[U];
        float b2[U][kGather ? W : 1], e2[U][W], c2[U][COLS ? W : 1], l2[U][COLS ? W : 1], g2[U][COLS ? W : 1];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            oth[u] = ((kGather || COLS) && valid[u]) ? ci[e[u]] : 0;
            pe[u] = COLS ? (valid[u] ? perm[e[u]] : 0) : e[u];   // the entry's position in A's arrays
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long c0 = (long long)h * a.tile;
            if constexpr (COLS) {
                attn_load<T, P>(c2[u], a.C + oth[u] * a.ldc + c0, n, t, valid[u]);
                attn_load<T, P>(l2[u], a.lse + oth[u] * a.ldlse + c0, n, t, valid[u]);
                attn_load<T, P>(g2[u], a.G + oth[u] * a.ldg + c0, n, t, valid[u]);
            } else if constexpr (kGather) {
                attn_load<T, P>(b2[u], a.B + oth[u] * a.ldb + c0, n, t, valid[u]);
            }
            attn_load<T, P>(e2[u], a.E + pe[u] * a.lde + c0, n, t, valid[u]);
        }
        if constexpr (PASS == kAttnForward) {
            float s[U][W];
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    e2[u][i] = edge_message<OP>(kGather ? b2[u][i] : 0.0f, e2[u][i]);   // (an entry the slot does not have: zeros in, 0 out)
                    s[u][i] = valid[u] ? score(e2[u][i], i) : -INFINITY;                // (exp gives those +0, and their messages are zero)
                }
            }
#pragma unroll
            for (int i = 0; i < W; ++i) {
                float mn = f[i];
#pragma unroll
                for (int u = 0; u < U; ++u) mn = fmaxf(mn, s[u][i]);
                const float mref = mn == -INFINITY ? 0.0f : mn;          // only -inf so far: everything stays +0
                const float al = softmax_exp(__fsub_rn(f[i], mref));   // 1 when m did not grow
                float zz = __fmul_rn(f[W + i], al), acc = __fmul_rn(f[2 * W + i], al);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const float w = softmax_exp(__fsub_rn(s[u][i], mref));
                    zz = __fadd_rn(zz, w);
                    acc = __fmaf_rn(w, e2[u][i], acc);
                }
                f[i] = mn; f[W + i] = zz; f[2 * W + i] = acc;
            }
        } else if constexpr (COLS) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!valid[u]) continue;
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    float gw, d;
                    const float q = grad(edge_message<OP>(x[i], e2[u][i]), c2[u][i], l2[u][i], g2[u][i], i, gw, d);
                    if (OP == kEdgeMul) f[i] = __fmaf_rn(q, e2[u][i], f[i]);
                    else if (OP == kEdgeAdd) f[i] = __fadd_rn(f[i], q);
                    else f[i] = __fadd_rn(f[i], __fadd_rn(x[i], e2[u][i]) > 0.0f ? q : 0.0f);
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float de[W];
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const float b = kGather ? b2[u][i] : 0.0f;
                    const float m = edge_message<OP>(b, e2[u][i]);
                    float gw, d;
                    const float q = grad(m, x[i], y[i], z[i], i, gw, d);
                    // floats beyond the tile and entries the slot does not have: the operands read as zero, so m = 0 and the term is +-0 --
                    // unless the row's own G is not finite; predicated all the same, as in SoftaggPass
                    const bool on = valid[u] && 4 * (t + T * (i / 4)) < n;
                    f[i] = on ? __fmaf_rn(gw, __fmul_rn(m, d), f[i]) : f[i];
                    de[i] = OP == kEdgeMul ? __fmul_rn(q, b) : OP == kEdgeAddRelu ? (__fadd_rn(b, e2[u][i]) > 0.0f ? q : 0.0f) : q;
                }
                if (a.dE && valid[u]) attn_store<T, P>(de, a.dE + pe[u] * a.ldde + (long long)h * a.tile, n, t);
            }
        }
    }

    // g <- g (+) o: SoftaggPass's own merge (the states have its layout) -- commutative operations only, so both sides of a butterfly
    // exchange compute the same bits
    static __device__ __forceinline__ void combine(float *g, const float *o) { SoftaggPass<PASS, T_, P_, U_>::combine(g, o); }

    // cnt: entries of the own row.  An empty row / column: +0 everywhere, lse = -inf
    __device__ __forceinline__ void finish(bool writer, int own, int cnt) {
        if (!writer) return;
        const long long r = own, c0 = (long long)h * a.tile;
        if (PASS == kAttnForward) {
            float c[W], l[W];
#pragma unroll
            for (int i = 0; i < W; ++i) {
                c[i] = cnt > 0 ? __fdiv_rn(f[2 * W + i], f[W + i]) : 0.0f;
                l[i] = cnt > 0 ? __fadd_rn(f[i], softagg_log(f[W + i])) : -INFINITY;
            }
            attn_store<T, P>(c, a.out + r * a.ldc + c0, n, t);
            if (a.out_lse) attn_store<T, P>(l, a.out_lse + r * a.ldlse + c0, n, t);
        } else if (PASS == kAttnBackwardRows) {
            if (!a.dt_rows) return;
            float d[W];
#pragma unroll
            for (int i = 0; i < W; ++i) d[i] = cnt > 0 ? f[i] : 0.0f;
            attn_store<T, P>(d, a.dt_rows + r * a.N + c0, n, t);
        } else {
            attn_store<T, P>(f, a.dB + r * a.lddb + c0, n, t);
        }
    }
};

}  // namespace sx
