// vector_attention_kernels.h -- channel-wise ("vector") attention from caller-supplied per-channel scores over a CSR pattern
// (sextans_vector_attention_device_rm / sextans_vector_attention_backward_device_rm): PointTransformerConv's
// x_i' = sum_j softmax_j(gamma(..))[n] * (W x_j + delta_ij)[n], DGL's edge_softmax on multi-channel edge data followed by u_mul_e_sum /
// e_mul_e, PyG's softmax(alpha, index) with a per-channel alpha.  The softmax of spmm_edge_softagg_kernels.h with the score DECOUPLED
// from the message: it is read from an (nnz, N) tensor of its own, never computed.  No counterpart in the reference.
//
//   m_e = V[c, n] (NODE) | V[c, n] + D[e, n] (ADD, ONE rounded add) | D[e, n] (EDGE, V is not read)
//   s_e = S[e, n]
//   forward        lse[r, n] = log sum_e exp(s_e);  w_e = exp(s_e - lse[r, n]);  C[r, n] = sum_e w_e m_e.  Empty row: C = +0, lse = -inf
//   backward, G the upstream gradient, gw_e = G[r, n] w_e:
//     rows             dS[e, n] = gw_e (m_e - C[r, n]) (+0 where s_e = -inf);  dD[e, n] = gw_e (ADD, EDGE), each stored once per (entry, tile)
//     cols (over A^T)  dV[c, n] = sum over the entries of column c of gw_e (NODE, ADD); EDGE has none
//
// Only A's PATTERN is read; S, D, dS and dD are (nnz, N) row-major in A's entry order, addressed as (long long)e * ld.  The passes plug
// into the row walking of pattern_pass.h as EdgeSoftaggPass does: COLUMN TILES of at most 64 floats play the heads' part, a slot of T
// lanes owns one (row, tile), the last tile of a row may be partial.
// The forward is SoftaggPass's online softmax with the score loaded instead of multiplied out: both call the one ChannelSoftmax of
// online_softmax.h (state, batch update, merge, the two results per float) -- so, fed S = t[n] m_e (one rounded product), it returns the
// bits of spmm_edge_softagg (ADD, EDGE) and of spmm_softagg on values of 1 (NODE).  A score of -inf masks its (entry, column): weight +0.
// The row pass keeps NO state (EdgePass's row pass): every (entry, tile) piece of dS and dD is stored by the slot that owns it, each
// store predicated on its pointer.  The column pass reads S through the transpose's permutation and gathers lse[r] and G[r]; it needs
// neither C, V nor D: the weight alone is dV's term.
// No atomics; sums in an order fixed by the pattern and the launch shape.
#pragma once
#include "online_softmax.h"

namespace sx {

enum { kVattNode = 1, kVattAdd = 2, kVattEdge = 3 };   // SEXTANS_VATT_*

// ET: the element type of the (nnz, N) tensors S, D, dS and dD in memory -- float, or uint16_t for bf16 (pattern_pass.h's typed attn_load /
// attn_store: fp32 in the registers either way).  The node tensors are fp32.
template <class ET>
struct VectorAttnArgsT {
    const ET *S;
    const float *V;             // not read by EDGE
    const ET *D;                // not read by NODE
    const float *C, *lse, *G;   // backward
    float *out, *out_lse;       // forward; out_lse may be null
    ET *dS;                     // backward, each may be null
    float *dV;
    ET *dD;
    long long lds, ldv, ldd, ldc, ldlse, ldg, ldds, lddv, lddd;
    int H;                      // column tiles (the bodies' "heads")
    int N, tile;                // tile: floats per tile = 4 T P
};
using VectorAttnArgs = VectorAttnArgsT<float>;

// the message: at most one rounded operation (the operand a mode does not read comes in as 0 and is not used)
template <int MSG>
__device__ __forceinline__ float vatt_message(float v, float d) {
    return MSG == kVattNode ? v : MSG == kVattAdd ? __fadd_rn(v, d) : d;
}

// One slot's view of a pass: the interface of AttnPass.  "own" is the row walked (the column pass: a column of A), ci[e] the other index.
template <int PASS, int MSG, int T_, int P_, int U_, class ET = float>
struct VectorAttnPass {
    using Args = VectorAttnArgsT<ET>;
    static constexpr int T = T_, P = P_, U = U_, W = 4 * P_;
    static constexpr int NF = PASS == kAttnForward ? 3 * W : PASS == kAttnBackwardCols ? W : 1;   // forward: m, z, acc per float; cols: dV
    static constexpr bool kMerge = PASS != kAttnBackwardRows;                                     // rows: nothing to merge
    static constexpr bool kV = MSG != kVattEdge, kD = MSG != kVattNode;                           // the message reads V / D
    const Args &a;
    const int *ci, *perm;
    const int t;
    int h = 0, n = 0;        // the tile and its valid floats
    float x[W], y[W], z[W];  // rows: the own row's C, lse and G
    float f[NF];

    __device__ __forceinline__ VectorAttnPass(const Args &a_, const int *ci_, const int *perm_, int t_)
        : a(a_), ci(ci_), perm(perm_), t(t_) {}

    __device__ __forceinline__ void begin(bool act, int own, int tile, bool) {
        h = tile;
        n = tile_floats(a, h);
        const long long r = act ? own : 0, c0 = (long long)h * a.tile;
        if (PASS == kAttnForward) {
            ChannelSoftmax<W>::init(f);
        } else {
            if (PASS == kAttnBackwardRows) {
                attn_load<T, P>(x, a.C + r * a.ldc + c0, n, t, act);
                attn_load<T, P>(y, a.lse + r * a.ldlse + c0, n, t, act);
                attn_load<T, P>(z, a.G + r * a.ldg + c0, n, t, act);
            }
#pragma unroll
            for (int i = 0; i < NF; ++i) f[i] = 0.0f;
        }
    }

    __device__ __forceinline__ void batch(const int (&e)[U_], const bool (&valid)[U_]) {
        constexpr bool COLS = PASS == kAttnBackwardCols;
        constexpr bool kGather = !COLS && kV;   // forward, rows: the entry's V row
        constexpr bool kEdge = !COLS && kD;     // forward, rows: the entry's D row
        long long oth[U], pe[U];
        float s2[U][W], v2[U][kGather ? W : 1], d2[U][kEdge ? W : 1], l2[U][COLS ? W : 1], g2[U][COLS ? W : 1];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            oth[u] = ((kGather || COLS) && valid[u]) ? ci[e[u]] : 0;
            pe[u] = COLS ? (valid[u] ? perm[e[u]] : 0) : e[u];   // the entry's position in A's arrays
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long c0 = (long long)h * a.tile;
            attn_load<T, P>(s2[u], a.S + pe[u] * a.lds + c0, n, t, valid[u]);
            if constexpr (COLS) {
                attn_load<T, P>(l2[u], a.lse + oth[u] * a.ldlse + c0, n, t, valid[u]);
                attn_load<T, P>(g2[u], a.G + oth[u] * a.ldg + c0, n, t, valid[u]);
            }
            if constexpr (kGather) attn_load<T, P>(v2[u], a.V + oth[u] * a.ldv + c0, n, t, valid[u]);
            if constexpr (kEdge) attn_load<T, P>(d2[u], a.D + pe[u] * a.ldd + c0, n, t, valid[u]);
        }
        if constexpr (PASS == kAttnForward) {
            float m2[U][W];
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    m2[u][i] = vatt_message<MSG>(kGather ? v2[u][i] : 0.0f, kEdge ? d2[u][i] : 0.0f);   // (an entry the slot does not have: 0)
                    s2[u][i] = valid[u] ? s2[u][i] : -INFINITY;                                           // (exp gives those +0)
                }
            }
            ChannelSoftmax<W>::template absorb<U>(f, s2, m2);
        } else if constexpr (COLS) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!valid[u]) continue;
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    // floats beyond the tile read s = lse = 0 and G = 0: the term is +0
                    f[i] = __fadd_rn(f[i], __fmul_rn(g2[u][i], softmax_exp(__fsub_rn(s2[u][i], l2[u][i]))));
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float ds[W], dd[W];
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const float m = vatt_message<MSG>(kGather ? v2[u][i] : 0.0f, kEdge ? d2[u][i] : 0.0f);
                    const float gw = __fmul_rn(z[i], softmax_exp(__fsub_rn(s2[u][i], y[i])));
                    dd[i] = gw;
                    ds[i] = s2[u][i] == -INFINITY ? 0.0f : __fmul_rn(gw, __fsub_rn(m, x[i]));   // a masked (entry, column): +0, not G's sign
                }
                if (!valid[u]) continue;
                const long long c0 = (long long)h * a.tile;
                if (a.dS) attn_store<T, P>(ds, a.dS + pe[u] * a.ldds + c0, n, t);
                if (kD && a.dD) attn_store<T, P>(dd, a.dD + pe[u] * a.lddd + c0, n, t);
            }
        }
    }

    // g <- g (+) o: the forward's state is ChannelSoftmax's, the column pass adds
    static __device__ __forceinline__ void combine(float *g, const float *o) {
        if constexpr (PASS == kAttnForward) ChannelSoftmax<W>::combine(g, o);
        else if constexpr (PASS == kAttnBackwardCols) state_add<NF>(g, o);
    }

    // cnt: entries of the own row.  An empty row / column: +0 everywhere, lse = -inf
    __device__ __forceinline__ void finish(bool writer, int own, int cnt) {
        if (!writer || PASS == kAttnBackwardRows) return;
        const long long r = own, c0 = (long long)h * a.tile;
        if (PASS == kAttnForward) {   // SoftaggFrame::finish's forward branch (online_softmax.h), kept inline: a helper around the two stores changes the kernels
            float c[W], l[W];
#pragma unroll
            for (int i = 0; i < W; ++i) {
                c[i] = ChannelSoftmax<W>::value(f, i, cnt);
                l[i] = ChannelSoftmax<W>::lse(f, i, cnt);
            }
            attn_store<T, P>(c, a.out + r * a.ldc + c0, n, t);
            if (a.out_lse) attn_store<T, P>(l, a.out_lse + r * a.ldlse + c0, n, t);
        } else {
            attn_store<T, P>(f, a.dV + r * a.lddv + c0, n, t);
        }
    }
};

}  // namespace sx
