// spmm_softagg_kernels.h -- softmax aggregation SpMM over a CSR matrix (sextans_spmm_softagg_device_rm /
// sextans_spmm_softagg_backward_device_rm): PyG's SoftmaxAggregation(t, learn=True), the aggregator of GENConv / DeeperGCN.  A softmax
// PER OUTPUT COLUMN over the row's messages themselves, with a temperature per column.  No counterpart in the reference.
//
//   p_e = val[e] * B[c, n]     s_e = t[n] * p_e   (t == NULL: s_e = p_e)      each ONE rounded fp32 multiply, never fused: the three
//                                                                              passes see the same bits of p and s
//   forward        lse[r, n] = log sum_e exp(s_e);  w_e = exp(s_e - lse[r, n]);  C[r, n] = sum_e w_e p_e.  Empty row: C = +0, lse = -inf
//   backward, G the upstream gradient, q_e = (G[r, n] w_e) (1 + t[n] (p_e - C[r, n])):
//     cols (over A^T)  dB[c, n] = sum over the entries of column c of val[e] q_e
//     rows             dval[e]  = sum_n B[c, n] q_e
//                      dt_rows[r, n] = G[r, n] sum_e w_e p_e (p_e - C[r, n]);  dt[n] = sum_r dt_rows[r, n]  (the two-level sum of GATv2's datt)
//
// The passes plug into the row walking of pattern_pass.h as ReducePass does: COLUMN TILES play the heads' part, a slot of T lanes owns
// one (row, tile), the last tile of a row may be partial.  The forward is the online softmax of attention_kernels.h per float instead of
// per head (ChannelSoftmax, online_softmax.h): its state is (m, z, acc) for every float, 3 W floats, and merging two states takes the
// larger m, rescales both sides and adds -- commutative operations only, so both sides of a butterfly end with the same bits.  A row of one entry ends with z = 1 and
// acc = p: C has the product's bits (a -0 product gives +0).  t p may be anything finite: only differences to the running maximum are
// exponentiated.  A non-finite product does what this arithmetic makes of it (inf - inf = NaN in its own (row, column)); it does not
// leave that (row, column).
// The row pass takes the tiles inside the slot ("heads_inside"): one lane owns dval[e] for every tile and adds the tiles in ascending
// order.  It ALWAYS keeps the row's dt sum in its state (W floats, merged by adds) and stores it when dt_rows is given: see
// engine_softagg.hip.  No atomics; sums in an order fixed by the pattern and the launch shape.
#pragma once
#include "online_softmax.h"

namespace sx {

struct SoftaggArgs {
    const float *val, *B, *t;   // val: nnz floats in A's entry order; t: N floats or null (= 1)
    const float *C, *lse, *G;   // backward
    float *out, *out_lse;       // forward; out_lse may be null
    float *dB, *dval, *dt_rows; // backward, each may be null; dt_rows: M x N floats, leading dimension N
    long long ldb, ldc, ldlse, ldg, lddb;
    int H;                      // column tiles (the bodies' "heads")
    int N, tile;                // tile: floats per tile = 4 T P
};

// One slot's view of a pass: the interface of AttnPass.  begin, score, grad, combine and finish are SoftaggFrame's (online_softmax.h).
template <int PASS, int T_, int P_, int U_>
struct SoftaggPass : SoftaggFrame<PASS, SoftaggArgs, T_, P_> {
    using Frame = SoftaggFrame<PASS, SoftaggArgs, T_, P_>;
    using Frame::Frame;
    using Frame::a, Frame::ci, Frame::perm, Frame::t, Frame::h, Frame::n, Frame::x, Frame::y, Frame::z, Frame::f, Frame::score, Frame::grad;
    static constexpr int T = T_, P = P_, U = U_, W = 4 * P_;

    __device__ __forceinline__ void batch(const int (&e)[U_], const bool (&valid)[U_]) {
        constexpr bool COLS = PASS == kAttnBackwardCols;
        long long oth[U];
        int pe[U];
        float v[U], p2[U][W], c2[U][COLS ? W : 1], l2[U][COLS ? W : 1], g2[U][COLS ? W : 1];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            oth[u] = valid[u] ? ci[e[u]] : 0;
            pe[u] = COLS ? (valid[u] ? perm[e[u]] : 0) : e[u];   // the entry's position in A's arrays
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long c0 = (long long)h * a.tile;
            if constexpr (COLS) {
                attn_load<T, P>(c2[u], a.C + oth[u] * a.ldc + c0, n, t, valid[u]);
                attn_load<T, P>(l2[u], a.lse + oth[u] * a.ldlse + c0, n, t, valid[u]);
                attn_load<T, P>(g2[u], a.G + oth[u] * a.ldg + c0, n, t, valid[u]);
            } else {
                attn_load<T, P>(p2[u], a.B + oth[u] * a.ldb + c0, n, t, valid[u]);
            }
            v[u] = valid[u] ? a.val[pe[u]] : 0.0f;
        }
        if constexpr (PASS == kAttnForward) {
            float s[U][W];
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    p2[u][i] = __fmul_rn(v[u], p2[u][i]);
                    s[u][i] = valid[u] ? score(p2[u][i], i) : -INFINITY;   // (exp gives those +0, and their products are zero)
                }
            }
            ChannelSoftmax<W>::template absorb<U>(f, s, p2);
        } else if constexpr (COLS) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!valid[u]) continue;
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    float gw, d;
                    const float q = grad(__fmul_rn(v[u], x[i]), c2[u][i], l2[u][i], g2[u][i], i, gw, d);
                    f[i] = __fmaf_rn(v[u], q, f[i]);
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float s = 0.0f;
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const float p = __fmul_rn(v[u], p2[u][i]);
                    float gw, d;
                    const float q = grad(p, x[i], y[i], z[i], i, gw, d);
                    // floats beyond the tile and entries the slot does not have: B = 0 or val = 0, so p = 0 and both terms are +-0 -- unless
                    // the row's own lse is -inf (an empty row has no entry) or G is not finite; predicated all the same
                    const bool on = valid[u] && 4 * (t + T * (i / 4)) < n;
                    s = on ? __fmaf_rn(p2[u][i], q, s) : s;
                    f[i] = on ? __fmaf_rn(gw, __fmul_rn(p, d), f[i]) : f[i];
                }
                if (a.dval) {
                    s = group_sum<T>(s);
                    // the tiles of an entry are taken by this lane one after the other, in ascending order: a plain read-modify-write
                    if (valid[u] && t == 0) a.dval[pe[u]] = h == 0 ? s : __fadd_rn(a.dval[pe[u]], s);
                }
            }
        }
    }
};

}  // namespace sx
