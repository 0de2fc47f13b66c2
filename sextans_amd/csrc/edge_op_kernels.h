// edge_op_kernels.h -- edge-OUTPUT ops from both endpoints of every stored entry of a CSR pattern (sextans_edge_op_device_rm /
// sextans_edge_op_backward_device_rm): DGL's gSDDMM half (u_add_v, u_sub_v, u_mul_v, copy_u, copy_v, each optionally + e), the glue in
// front of the families that READ an (nnz, N) tensor -- Point Transformer's phi(x_i) - psi(x_j) + delta_ij, EdgeConv's x_j - x_i,
// MeshGraphNets' concat(e, x_i, x_j), GatedGCN's pre-activations without the aggregation.  No counterpart in the reference.
//
//   forward       z = x_dst[r, n] + | - | * x_src[c, n]  |  x_dst[r, n]  |  x_src[c, n]        (ONE rounded fp32 operation)
//                 Z[e, n] = z, or z + E[e, n] (a second rounded add, in this order) when E is given
//   endpoint sum  out[own, n] = sum over the own row's entries of Gz[e, n] (PLAIN), of -Gz[e, n] (NEG: f - g from +0) or of
//                 Gz[e, n] * x[oth, n] (MUL: fmaf).  On A's arrays: own = r, oth = c, e the entry itself -- dx_dst.  On A^T's arrays with
//                 the transpose's permutation: own = c, oth = r, e = perm[.] -- dx_src.  ONE pass type serves both.
//
// Only A's PATTERN is read; Z, E and Gz are (nnz, N) row-major in A's entry order, addressed as (long long)e * ld.  The passes plug into
// the row walking of pattern_pass.h as EdgePass does: COLUMN TILES of at most 128 floats play the heads' part, a slot of T lanes owns one
// (row, tile), lane t holds the 16-byte pieces t, t + T, .. of the tile, the last tile of a row may be partial (pieces beyond N
// predicated off).  The forward keeps NO state (EdgePass's row pass): the own row's pieces sit in registers from begin(), every
// (entry, tile) piece of Z is stored by the slot that owns it.  The endpoint sum's state is the tile's partial sums, merged by
// __fadd_rn.  No atomics; sums in an order fixed by the pattern and the launch shape.
#pragma once
#include "pattern_pass.h"

namespace sx {

enum { kEdgeOpAdd = 1, kEdgeOpSub = 2, kEdgeOpMul = 3, kEdgeOpDst = 4, kEdgeOpSrc = 5 };   // SEXTANS_EDGEOP_*
enum { kEndSumPlain = 0, kEndSumNeg = 1, kEndSumMul = 2 };                                  // the endpoint sum's term

// ET: the element type of the (nnz, N) tensors E, Z and Gz in memory -- float, or uint16_t for bf16 (pattern_pass.h's typed attn_load /
// attn_store: fp32 in the registers either way).  The node tensors are fp32.
template <class ET>
struct EdgeOpArgsT {
    const float *xdst, *xsrc;       // forward
    const ET *E;
    ET *Z;
    const ET *Gz;                   // endpoint sum
    const float *x;                 //   x: the OTHER endpoint's rows (MUL)
    float *out;
    long long ldxdst, ldxsrc, lde, ldz, ldgz, ldx, ldout;
    int H;                          // column tiles (the bodies' "heads")
    int N, tile;                    // tile: floats per tile = 4 T P
};
using EdgeOpArgs = EdgeOpArgsT<float>;

// The forward: "own" is the row r of A, ci[e] the column c.  HAS_E: E is given.
template <int OP, bool HAS_E, int T_, int P_, int U_, class ET = float>
struct EdgeOpPass {
    using Args = EdgeOpArgsT<ET>;
    static constexpr int T = T_, P = P_, U = U_, W = 4 * P_;
    static constexpr int NF = 1;           // nothing to merge
    static constexpr bool kMerge = false;
    static constexpr bool kDst = OP != kEdgeOpSrc, kSrc = OP != kEdgeOpDst;   // what the op reads
    const Args &a;
    const int *ci, *perm;
    const int t;
    int h = 0, n = 0;   // the tile and its valid floats
    float y[W];         // the own row's x_dst
    float f[NF];

    __device__ __forceinline__ EdgeOpPass(const Args &a_, const int *ci_, const int *perm_, int t_) : a(a_), ci(ci_), perm(perm_), t(t_) {}

    __device__ __forceinline__ void begin(bool act, int own, int tile, bool) {
        h = tile;
        n = min(a.tile, a.N - h * a.tile);
        const long long r = act ? own : 0;
        if (kDst) attn_load<T, P>(y, a.xdst + r * a.ldxdst + (long long)h * a.tile, n, t, act);
    }

    __device__ __forceinline__ void batch(const int (&e)[U_], const bool (&valid)[U_]) {
        const long long c0 = (long long)h * a.tile;
        long long oth[U];
        float g[U][kSrc ? W : 1], x[U][HAS_E ? W : 1];
#pragma unroll
        for (int u = 0; u < U; ++u) oth[u] = (kSrc && valid[u]) ? ci[e[u]] : 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (kSrc) attn_load<T, P>(g[u], a.xsrc + oth[u] * a.ldxsrc + c0, n, t, valid[u]);
            if (HAS_E) attn_load<T, P>(x[u], a.E + (long long)e[u] * a.lde + c0, n, t, valid[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!valid[u]) continue;
            float z[W];
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const float s = kSrc ? g[u][i] : 0.0f;
                z[i] = OP == kEdgeOpAdd ? __fadd_rn(y[i], s) : OP == kEdgeOpSub ? __fsub_rn(y[i], s) : OP == kEdgeOpMul ? __fmul_rn(y[i], s)
                     : OP == kEdgeOpDst ? y[i] : s;
                if (HAS_E) z[i] = __fadd_rn(z[i], x[u][i]);
            }
            attn_store<T, P>(z, a.Z + (long long)e[u] * a.ldz + c0, n, t);
        }
    }

    static __device__ __forceinline__ void combine(float *, const float *) {}
    __device__ __forceinline__ void finish(bool, int, int) {}
};

// The endpoint sum: "own" is the row walked (with PERM: a column of A, walked as a row of A^T), ci[e] the other index, perm[e] the
// entry's position in A's arrays.
template <int TERM, bool PERM, int T_, int P_, int U_, class ET = float>
struct EndpointSumPass {
    using Args = EdgeOpArgsT<ET>;
    static constexpr int T = T_, P = P_, U = U_, W = 4 * P_;
    static constexpr int NF = W;
    static constexpr bool kMerge = true;
    static constexpr bool kGather = TERM == kEndSumMul;   // the other endpoint's row
    const Args &a;
    const int *ci, *perm;
    const int t;
    int h = 0, n = 0;   // the tile and its valid floats
    float f[NF];

    __device__ __forceinline__ EndpointSumPass(const Args &a_, const int *ci_, const int *perm_, int t_) : a(a_), ci(ci_), perm(perm_), t(t_) {}

    __device__ __forceinline__ void begin(bool, int, int tile, bool) {
        h = tile;
        n = min(a.tile, a.N - h * a.tile);
#pragma unroll
        for (int i = 0; i < NF; ++i) f[i] = 0.0f;
    }

    __device__ __forceinline__ void batch(const int (&e)[U_], const bool (&valid)[U_]) {
        const long long c0 = (long long)h * a.tile;
        long long oth[U], pe[U];
        float g[U][W], x[U][kGather ? W : 1];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            oth[u] = (kGather && valid[u]) ? ci[e[u]] : 0;
            pe[u] = PERM ? (valid[u] ? perm[e[u]] : 0) : e[u];   // the entry's position in A's arrays
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            attn_load<T, P>(g[u], a.Gz + pe[u] * a.ldgz + c0, n, t, valid[u]);
            if (kGather) attn_load<T, P>(x[u], a.x + oth[u] * a.ldx + c0, n, t, valid[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!valid[u]) continue;
#pragma unroll
            for (int i = 0; i < W; ++i) {
                f[i] = TERM == kEndSumMul ? __fmaf_rn(g[u][i], x[u][i], f[i]) : TERM == kEndSumNeg ? __fsub_rn(f[i], g[u][i]) : __fadd_rn(f[i], g[u][i]);
            }
        }
    }

    static __device__ __forceinline__ void combine(float *g, const float *o) {
#pragma unroll
        for (int i = 0; i < NF; ++i) g[i] = __fadd_rn(g[i], o[i]);
    }

    // an empty row / column: +0 everywhere
    __device__ __forceinline__ void finish(bool writer, int own, int) {
        if (!writer) return;
        attn_store<T, P>(f, a.out + (long long)own * a.ldout + (long long)h * a.tile, n, t);
    }
};

}  // namespace sx
