// spmm_reduce_kernels.h -- max / min aggregation SpMM over a CSR matrix (sextans_spmm_reduce_device_rm /
// sextans_spmm_reduce_backward_device_rm): what torch.sparse.mm(A, B, "amax" / "amin") computes on the CPU.  No counterpart in the
// reference: its PEs only multiply and accumulate.
//
//   forward        p_e = val[e] * B[c, n]  (one rounded fp32 product, never fused);  C[r, n] = max / min over the row's entries of p_e
//                  arg[r, n] = the winning entry's position in A's arrays: NaN beats every number, then the better product, then the
//                  SMALLER position (+0 == -0) -- np.argmax / np.argmin over the row's product block.  Empty row: C = +0, arg = -1
//   backward cols  (over A^T)  dB[c, n] = sum over the entries e of column c with arg[r, n] == e of val[e] * G[r, n]
//   backward rows  dval[e] = sum over the n with arg[r, n] == e of G[r, n] * B[c, n]
//
// The passes below plug into the row walking of pattern_pass.h (attn_rows_body, attn_long_body) exactly as GatPass does; COLUMN
// TILES of at most 128 floats play the heads' part: a slot of T lanes owns one (row, tile), lane t holds the 16-byte pieces t, t + T, ..
// of the tile, the last tile of a row may be partial (pieces beyond N predicated off).  The forward's partial state per float is
// (best product, best position), the position kept in f[] as its bit pattern so that the bodies' shuffles and LDS merge move it like
// any float.  Merging two states is the same lexicographic comparison the entries go through, which is associative and commutative:
// any split of a row over slots, wavefronts and the long-row workgroup gives the same bits, the winner included.
// The backward passes gather: the column pass reads arg and G of an entry's row and adds where the entry won, the row pass (tiles inside
// the slot, "heads_inside") sums the selected G * B over its pieces and a butterfly; one lane owns dval[e] for every tile and adds the
// tiles in ascending order.  No atomics; sums in an order fixed by the pattern and the launch shape.
#pragma once
#include "pattern_pass.h"

namespace sx {

enum { kReduceMax = 1, kReduceMin = 2 };   // SEXTANS_REDUCE_*

struct ReduceArgs {
    const float *val, *B, *G;   // val: nnz floats in A's entry order
    const int *arg;             // backward
    float *C, *dB, *dval;
    int *out_arg;               // forward: may be null
    long long ldb, ldc, ldarg, ldg, lddb;
    int H;                      // column tiles (the bodies' "heads")
    int N, tile;                // tile: floats per tile = 4 T P
};

template <int T, int P>
__device__ __forceinline__ void reduce_load_arg(int *x, const int *row, int n, int t, bool ok) {   // as attn_load; -1 beyond n
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int col = 4 * (t + T * k);
        int4 v = make_int4(-1, -1, -1, -1);
        if (ok && col < n) v = *reinterpret_cast<const int4 *>(row + col);
        x[4 * k] = v.x; x[4 * k + 1] = v.y; x[4 * k + 2] = v.z; x[4 * k + 3] = v.w;
    }
}

// does (p, e) come before (q, i)?  NaN first, then the better product, then the smaller position.  (q, i) may be the start state
// (-inf / +inf, INT_MAX), which every entry beats
template <int OP>
__device__ __forceinline__ bool reduce_wins(float p, int e, float q, int i) {
    const bool pn = p != p, qn = q != q;
    if (pn || qn) return pn && (!qn || e < i);
    return (OP == kReduceMax ? p > q : p < q) || (p == q && e < i);
}

// One slot's view of a pass: the interface of AttnPass.  OP matters to the forward only.
template <int PASS, int OP, int T_, int P_, int U_>
struct ReducePass {
    using Args = ReduceArgs;
    static constexpr int T = T_, P = P_, U = U_, W = 4 * P_;
    static constexpr int NF = PASS == kAttnForward ? 2 * W : PASS == kAttnBackwardRows ? 1 : W;   // forward: best, position; rows: nothing to merge; cols: dB
    static constexpr bool kMerge = PASS != kAttnBackwardRows;
    const ReduceArgs &a;
    const int *ci, *perm;
    const int t;
    int h = 0, n = 0;   // the tile and its valid floats
    int x[W];           // rows: the own row's arg
    float y[W];         // rows: the own row's G
    float f[NF];

    __device__ __forceinline__ ReducePass(const ReduceArgs &a_, const int *ci_, const int *perm_, int t_) : a(a_), ci(ci_), perm(perm_), t(t_) {}

    __device__ __forceinline__ void begin(bool act, int own, int tile, bool) {
        h = tile;
        n = min(a.tile, a.N - h * a.tile);
        const long long r = act ? own : 0;
        if (PASS == kAttnForward) {
#pragma unroll
            for (int i = 0; i < W; ++i) {
                f[i] = OP == kReduceMax ? -INFINITY : INFINITY;
                f[W + i] = __int_as_float(INT_MAX);
            }
        } else if (PASS == kAttnBackwardRows) {
            reduce_load_arg<T, P>(x, a.arg + r * a.ldarg + (long long)h * a.tile, n, t, act);
            attn_load<T, P>(y, a.G + r * a.ldg + (long long)h * a.tile, n, t, act);
            f[0] = 0.0f;
        } else {
#pragma unroll
            for (int i = 0; i < NF; ++i) f[i] = 0.0f;
        }
    }

    __device__ __forceinline__ void batch(const int (&e)[U_], const bool (&valid)[U_]) {
        long long oth[U];
        int pe[U], q[U][PASS == kAttnBackwardCols ? W : 1];
        float v[U], p2[U][W];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            oth[u] = valid[u] ? ci[e[u]] : 0;
            pe[u] = PASS == kAttnBackwardCols ? (valid[u] ? perm[e[u]] : 0) : e[u];   // the entry's position in A's arrays
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (PASS == kAttnBackwardCols) {
                reduce_load_arg<T, P>(q[u], a.arg + oth[u] * a.ldarg + (long long)h * a.tile, n, t, valid[u]);
                attn_load<T, P>(p2[u], a.G + oth[u] * a.ldg + (long long)h * a.tile, n, t, valid[u]);
            } else {
                attn_load<T, P>(p2[u], a.B + oth[u] * a.ldb + (long long)h * a.tile, n, t, valid[u]);
            }
            v[u] = (PASS != kAttnBackwardRows && valid[u]) ? a.val[pe[u]] : 0.0f;
        }
        if (PASS == kAttnForward) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!valid[u]) continue;
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const float p = __fmul_rn(v[u], p2[u][i]);
                    if (reduce_wins<OP>(p, pe[u], f[i], __float_as_int(f[W + i]))) {
                        f[i] = p;
                        f[W + i] = __int_as_float(pe[u]);
                    }
                }
            }
        } else if (PASS == kAttnBackwardCols) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!valid[u]) continue;
#pragma unroll
                for (int i = 0; i < W; ++i)
                    if (q[u][i] == pe[u]) f[i] = __fmaf_rn(v[u], p2[u][i], f[i]);
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float s = 0.0f;
#pragma unroll
                for (int i = 0; i < W; ++i)
                    if (x[i] == pe[u]) s = __fmaf_rn(y[i], p2[u][i], s);
                s = group_sum<T>(s);
                // the tiles of an entry are taken by this lane one after the other, in ascending order: a plain read-modify-write
                if (valid[u] && t == 0) a.dval[pe[u]] = h == 0 ? s : __fadd_rn(a.dval[pe[u]], s);
            }
        }
    }

    // g <- g (+) o: both sides of a butterfly exchange end with the same bits (the comparison is a total order on distinct positions)
    static __device__ __forceinline__ void combine(float *g, const float *o) {
        if (PASS == kAttnForward) {
#pragma unroll
            for (int i = 0; i < W; ++i) {
                if (reduce_wins<OP>(o[i], __float_as_int(o[W + i]), g[i], __float_as_int(g[W + i]))) {
                    g[i] = o[i];
                    g[W + i] = o[W + i];
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
        const long long r = own;
        if (PASS == kAttnForward) {
            float c[W];
            int g[W];
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const int idx = __float_as_int(f[W + i]);
                c[i] = idx == INT_MAX ? 0.0f : f[i];
                g[i] = idx == INT_MAX ? -1 : idx;
            }
            attn_store<T, P>(c, a.C + r * a.ldc + (long long)h * a.tile, n, t);
            if (a.out_arg) {
                int *row = a.out_arg + r * a.ldarg + (long long)h * a.tile;
#pragma unroll
                for (int k = 0; k < P; ++k) {
                    const int col = 4 * (t + T * k);
                    if (col < n) *reinterpret_cast<int4 *>(row + col) = make_int4(g[4 * k], g[4 * k + 1], g[4 * k + 2], g[4 * k + 3]);
                }
            }
        } else {
            attn_store<T, P>(f, a.dB + r * a.lddb + (long long)h * a.tile, n, t);
        }
    }
};

}  // namespace sx
