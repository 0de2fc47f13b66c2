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
// The forward is SoftaggPass's online softmax with another source of the message: both passes are SoftaggFrame (online_softmax.h) plus
// a batch() that hands its scores and messages to the one ChannelSoftmax -- so with E[e, :] = val[e] and MUL it returns spmm_softagg's bits.
// The row pass does NOT take the tiles inside the slot (there is no dval to add up over tiles): every (entry, tile) piece of dE is stored
// by the slot that owns it, as in EdgePass; its state is the tile's dt sum (W floats, merged by adds), kept whether or not dt is asked
// for and stored when dt_rows is given; the dE store is predicated on its pointer (edge_softagg_launch.h says why).
// No atomics; sums in an order fixed by the pattern and the launch shape.
#pragma once
#include "spmm_edge_kernels.h"
#include "spmm_softagg_kernels.h"

namespace sx {

// ET: the element type of the (nnz, N) tensors E and dE in memory -- float, or uint16_t for bf16 (pattern_pass.h's typed attn_load /
// attn_store: fp32 in the registers either way).  The node tensors, t and dt_rows are fp32.
template <class ET>
struct EdgeSoftaggArgsT {
    const float *B;
    const ET *E;
    const float *t;             // N floats or null (= 1)
    const float *C, *lse, *G;   // backward
    float *out, *out_lse;       // forward; out_lse may be null
    float *dB;                  // backward, each may be null
    ET *dE;
    float *dt_rows;             // M x N floats, leading dimension N
    long long ldb, lde, ldc, ldlse, ldg, lddb, ldde;
    int H;                      // column tiles (the bodies' "heads")
    int N, tile;                // tile: floats per tile = 4 T P
};
using EdgeSoftaggArgs = EdgeSoftaggArgsT<float>;

// the message of spmm_edge_kernels.h: one rounded operation (b is not read for COPY)
template <int OP>
__device__ __forceinline__ float edge_message(float b, float x) {
    return OP == kEdgeMul ? __fmul_rn(b, x) : OP == kEdgeAdd ? __fadd_rn(b, x) : OP == kEdgeAddRelu ? edge_relu(__fadd_rn(b, x)) : x;
}

// One slot's view of a pass: the interface of AttnPass.  "own" is the row walked (the column pass: a column of A), ci[e] the other index.
// begin, score, grad, combine and finish are SoftaggFrame's (online_softmax.h), the ones SoftaggPass has.
template <int PASS, int OP, int T_, int P_, int U_, class ET = float>
struct EdgeSoftaggPass : SoftaggFrame<PASS, EdgeSoftaggArgsT<ET>, T_, P_> {
    using Frame = SoftaggFrame<PASS, EdgeSoftaggArgsT<ET>, T_, P_>;
    using Frame::Frame;
    using Frame::a, Frame::ci, Frame::perm, Frame::t, Frame::h, Frame::n, Frame::x, Frame::y, Frame::z, Frame::f, Frame::score, Frame::grad;
    static constexpr int T = T_, P = P_, U = U_, W = 4 * P_;
    static constexpr bool kB = OP != kEdgeCopy;   // the message reads B

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
            ChannelSoftmax<W>::template absorb<U>(f, s, e2);
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
};

}  // namespace sx
