// spmm_edge_kernels.h -- SpMM with a feature VECTOR per stored entry (sextans_spmm_edge_device_rm / sextans_spmm_edge_backward_device_rm):
// continuous-filter convolution (u_mul_e_sum), GINE (relu(u_add_e) summed), edge -> node reduction (copy_e_sum).  No counterpart in the
// reference: its PEs weight an entry with a scalar.
//
//   forward        m[e, n] = B[c, n] * E[e, n] | B[c, n] + E[e, n] | relu(B[c, n] + E[e, n]) | E[e, n]   (one rounded fp32 operation)
//                  C[r, n] = sum over the row's entries of m[e, n]   (__fadd_rn; an empty row: +0)
//   backward cols  (over A^T)  dB[c, n] = sum over the entries of column c of G[r, n] * E[e, n] | G[r, n] | (B + E > 0 ? G[r, n] : 0)
//   backward rows  dE[e, n] = G[r, n] * B[c, n] | G[r, n] | (B + E > 0 ? G[r, n] : +0) | G[r, n]   (one rounded operation, stored directly)
//
// Only A's PATTERN is read; E and dE are (nnz, N) row-major in A's entry order, addressed as (long long)e * ld.  The passes plug into the
// row walking of pattern_pass.h (attn_rows_body, attn_long_body) as ReducePass does; COLUMN TILES of at most 128 floats play the
// heads' part: a slot of T lanes owns one (row, tile), lane t holds the 16-byte pieces t, t + T, .. of the tile, the last tile of a row
// may be partial (pieces beyond N predicated off).  The forward's and the column pass's state is the tile's partial sums, merged by
// __fadd_rn; the row pass has no state: each (entry, tile) belongs to one slot, which stores its dE piece.  No atomics; sums in an order
// fixed by the pattern and the launch shape.
#pragma once
#include "pattern_pass.h"

namespace sx {

enum { kEdgeMul = 1, kEdgeAdd = 2, kEdgeAddRelu = 3, kEdgeCopy = 4 };   // SEXTANS_EDGE_*

// ET: the element type of the (nnz, N) tensors E and dE in memory -- float, or uint16_t for bf16 (pattern_pass.h's typed attn_load /
// attn_store: fp32 in the registers either way).  The node tensors are fp32.
template <class ET>
struct EdgeArgsT {
    const float *B;
    const ET *E;
    const float *G;
    float *C, *dB;
    ET *dE;
    long long ldb, lde, ldc, ldg, lddb, ldde;
    int H;                      // column tiles (the bodies' "heads")
    int N, tile;                // tile: floats per tile = 4 T P
};
using EdgeArgs = EdgeArgsT<float>;

// relu that keeps a NaN and gives +0 for everything else that is not positive
__device__ __forceinline__ float edge_relu(float s) { return s > 0.0f ? s : (s != s ? s : 0.0f); }

// One slot's view of a pass: the interface of AttnPass.  "own" is the row walked (the column pass: a column of A), ci[e] the other index.
template <int PASS, int OP, int T_, int P_, int U_, class ET = float>
struct EdgePass {
    using Args = EdgeArgsT<ET>;
    static constexpr int T = T_, P = P_, U = U_, W = 4 * P_;
    static constexpr int NF = PASS == kAttnBackwardRows ? 1 : W;   // forward: C's sums; cols: dB's; rows: nothing to merge
    static constexpr bool kMerge = PASS != kAttnBackwardRows;
    // what an entry reads besides the own row's vector
    static constexpr bool kGather = PASS == kAttnForward ? OP != kEdgeCopy                               // B[c]
                                  : PASS == kAttnBackwardCols ? true                                       // G[r]
                                  : (OP == kEdgeMul || OP == kEdgeAddRelu);                                // B[c]
    static constexpr bool kEdge = PASS == kAttnForward ? true : PASS == kAttnBackwardCols ? OP != kEdgeAdd : OP == kEdgeAddRelu;   // E[e]
    const Args &a;
    const int *ci, *perm;
    const int t;
    int h = 0, n = 0;   // the tile and its valid floats
    float y[W];         // rows: the own row's G; cols with ADD_RELU: the own column's B
    float f[NF];

    __device__ __forceinline__ EdgePass(const Args &a_, const int *ci_, const int *perm_, int t_) : a(a_), ci(ci_), perm(perm_), t(t_) {}

    __device__ __forceinline__ void begin(bool act, int own, int tile, bool) {
        h = tile;
        n = min(a.tile, a.N - h * a.tile);
        const long long r = act ? own : 0;
        if (PASS == kAttnBackwardRows) attn_load<T, P>(y, a.G + r * a.ldg + (long long)h * a.tile, n, t, act);
        else if (PASS == kAttnBackwardCols && OP == kEdgeAddRelu) attn_load<T, P>(y, a.B + r * a.ldb + (long long)h * a.tile, n, t, act);
#pragma unroll
        for (int i = 0; i < NF; ++i) f[i] = 0.0f;
    }

    __device__ __forceinline__ void batch(const int (&e)[U_], const bool (&valid)[U_]) {
        long long oth[U], pe[U];
        float g[U][kGather ? W : 1], x[U][kEdge ? W : 1];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            oth[u] = (kGather && valid[u]) ? ci[e[u]] : 0;
            pe[u] = PASS == kAttnBackwardCols ? ((kEdge && valid[u]) ? perm[e[u]] : 0) : e[u];   // the entry's position in A's arrays
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (kGather) {
                const float *src = PASS == kAttnBackwardCols ? a.G + oth[u] * a.ldg : a.B + oth[u] * a.ldb;
                attn_load<T, P>(g[u], src + (long long)h * a.tile, n, t, valid[u]);
            }
            if (kEdge) attn_load<T, P>(x[u], a.E + pe[u] * a.lde + (long long)h * a.tile, n, t, valid[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!valid[u]) continue;
            if (PASS == kAttnForward) {
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const float m = OP == kEdgeMul ? __fmul_rn(g[u][i], x[u][i]) : OP == kEdgeAdd ? __fadd_rn(g[u][i], x[u][i])
                                  : OP == kEdgeAddRelu ? edge_relu(__fadd_rn(g[u][i], x[u][i])) : x[u][i];
                    f[i] = __fadd_rn(f[i], m);
                }
            } else if (PASS == kAttnBackwardCols) {
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    if (OP == kEdgeMul) f[i] = __fmaf_rn(g[u][i], x[u][i], f[i]);
                    else if (OP == kEdgeAdd) f[i] = __fadd_rn(f[i], g[u][i]);
                    else f[i] = __fadd_rn(f[i], __fadd_rn(y[i], x[u][i]) > 0.0f ? g[u][i] : 0.0f);
                }
            } else {
                float d[W];
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    d[i] = OP == kEdgeMul ? __fmul_rn(y[i], g[u][i]) : OP == kEdgeAddRelu ? (__fadd_rn(g[u][i], x[u][i]) > 0.0f ? y[i] : 0.0f) : y[i];
                }
                attn_store<T, P>(d, a.dE + pe[u] * a.ldde + (long long)h * a.tile, n, t);
            }
        }
    }

    static __device__ __forceinline__ void combine(float *g, const float *o) {
        if (PASS == kAttnBackwardRows) return;
#pragma unroll
        for (int i = 0; i < NF; ++i) g[i] = __fadd_rn(g[i], o[i]);
    }

    __device__ __forceinline__ void finish(bool writer, int own, int) {
        if (!writer || PASS == kAttnBackwardRows) return;
        const long long r = own;
        if (PASS == kAttnForward) attn_store<T, P>(f, a.C + r * a.ldc + (long long)h * a.tile, n, t);
        else attn_store<T, P>(f, a.dB + r * a.lddb + (long long)h * a.tile, n, t);
    }
};

}  // namespace sx
