// spmm_gated_kernels.h -- gated aggregation over a CSR pattern (sextans_spmm_gated_device_rm / sextans_spmm_gated_backward_device_rm):
// the message passing of ResGatedGraphConv (PyG) and GatedGCN (Bresson & Laurent; the MPNN of GraphGPS).  Every stored entry gets a
// per-channel sigmoid gate from both endpoints and, optionally, its own features.  No counterpart in the reference.
//
//   z_e[n] = (xdst[r, n] + xsrc[c, n]) + E[e, n]     two rounded fp32 adds in this order; without E the first one alone
//   g_e[n] = gate_sigmoid(z_e[n])                    the SAME function in the three passes: the backward recomputes the forward's bits
//   forward        num[r, n] = sum_e fma(g_e, V[c, n], num)   den[r, n] = sum_e g_e   (__fadd_rn merges; an empty row: both +0)
//                  C = num (SUM) | num / (den + eps) (NORM);  z_e is stored when asked for: the layer's new edge features
//   backward, gn = G (SUM) | G / (den + eps) (NORM, written once by engine_gated.hip's gated_gn), C == 0 in SUM:
//                  dg = gn (v - C)     dz_e = fma(dg, g (1 - g), Gz[e])      (Gz: the upstream gradient of the z output, or absent)
//     rows         dE[e, n] = dz_e (one store per (entry, tile));  dxdst[r, n] = sum_e dz_e
//     cols (A^T)   dxsrc[c, n] = sum over the entries of column c of dz_e;  dV[c, n] = sum of fma(g_e, gn[r, n], dV)
//
// Only A's PATTERN is read; E, z, Gz and dE are (nnz, N) row-major in A's entry order, addressed as (long long)e * ld.  The passes plug
// into the row walking of pattern_pass.h as EdgePass does: COLUMN TILES of at most 64 floats play the heads' part and sit in the grid in
// every pass, a slot of T lanes owns one (row, tile), the last tile of a row may be partial.  E, Gz, the z output, the mode and the
// optional outputs are uniform run-time branches on the argument block: one kernel per pass and width.  No atomics; sums in an order fixed
// by the pattern and the launch shape.
#pragma once
#include "pattern_pass.h"

namespace sx {

// ET: the element type of the (nnz, N) tensors E, z, Gz and dE in memory -- float, or uint16_t for bf16 (pattern_pass.h's typed attn_load /
// attn_store: fp32 in the registers either way, a bf16 store rounds its copy only).  Everything of node size is fp32.
template <class ET>
struct GatedArgsT {
    const float *xdst, *xsrc, *V;
    const ET *E;                               // may be null
    const float *C, *gn;                       // backward; C null: SUM mode (C == 0)
    const ET *Gz;                              // backward; may be null
    float *out, *den;                          // forward; den may be null
    ET *z;                                     // forward; may be null
    float *dxdst, *dxsrc, *dV;                 // backward, each may be null
    ET *dE;
    long long ld_xdst, ld_xsrc, ld_v, ld_e, ldc, ldden, ldz, ldgn, ldgz, ld_dxdst, ld_dxsrc, ld_dv, ld_de;
    float eps;
    int norm;                                  // forward: C = num / (den + eps)
    int H;                                     // column tiles (the bodies' "heads")
    int N, tile;                               // tile: floats per tile = 4 T P
};
using GatedArgs = GatedArgsT<float>;

// 1 / (1 + exp(-z)), the division rounded to nearest: exactly 1 once exp(-z) vanishes against 1 (z >= 17), exactly +0 once it overflows
// (z <= -89: 1 / inf), never inf; a NaN stays one.
__device__ __forceinline__ float gate_sigmoid(float z) { return __fdiv_rn(1.0f, __fadd_rn(1.0f, softmax_exp(-z))); }

// z of an entry: (own + other) is commutative, so the row passes (own = xdst) and the column pass (own = xsrc) give the same bits
__device__ __forceinline__ float gate_z(float a, float b, float e, bool has_e) {
    const float s = __fadd_rn(a, b);
    return has_e ? __fadd_rn(s, e) : s;
}
// dz from the recomputed gate: gn (v - c) g (1 - g) (+ gz)
__device__ __forceinline__ float gate_dz(float g, float gn, float v, float c, float gz, bool has_gz) {
    const float dg = __fmul_rn(gn, __fsub_rn(v, c)), s = __fmul_rn(g, __fsub_rn(1.0f, g));
    return has_gz ? __fmaf_rn(dg, s, gz) : __fmul_rn(dg, s);
}

// One slot's view of a pass: the interface of AttnPass.  "own" is the row walked (the column pass: a column of A), ci[e] the other index.
template <int PASS, int T_, int P_, int U_, class ET = float>
struct GatedPass {
    using Args = GatedArgsT<ET>;
    static constexpr int T = T_, P = P_, U = U_, W = 4 * P_;
    static constexpr bool kCols = PASS == kAttnBackwardCols;
    static constexpr int NF = PASS == kAttnBackwardRows ? W : 2 * W;   // forward: num, den; rows: dxdst; cols: dV, dxsrc
    static constexpr bool kMerge = true;
    const Args &a;
    const int *ci, *perm;
    const int t;
    int h = 0, n = 0;                       // the tile and its valid floats
    float x[W];                             // the own row's xdst (cols: the own column's xsrc)
    float y[PASS == kAttnForward ? 1 : W];  // rows: the own row's gn; cols: the own column's V
    float c[PASS == kAttnBackwardRows ? W : 1];   // rows: the own row's C (SUM: 0)
    float f[NF];

    __device__ __forceinline__ GatedPass(const Args &a_, const int *ci_, const int *perm_, int t_) : a(a_), ci(ci_), perm(perm_), t(t_) {}

    __device__ __forceinline__ void begin(bool act, int own, int tile, bool) {
        h = tile;
        n = min(a.tile, a.N - h * a.tile);
        const long long r = act ? own : 0, c0 = (long long)h * a.tile;
        if (kCols) {
            attn_load<T, P>(x, a.xsrc + r * a.ld_xsrc + c0, n, t, act);
            attn_load<T, P>(y, a.V + r * a.ld_v + c0, n, t, act);
        } else {
            attn_load<T, P>(x, a.xdst + r * a.ld_xdst + c0, n, t, act);
            if (PASS == kAttnBackwardRows) {
                attn_load<T, P>(y, a.gn + r * a.ldgn + c0, n, t, act);
                attn_load<T, P>(c, a.C + r * a.ldc + c0, n, t, act && a.C);
            }
        }
#pragma unroll
        for (int i = 0; i < NF; ++i) f[i] = 0.0f;
    }

    __device__ __forceinline__ void batch(const int (&e)[U_], const bool (&valid)[U_]) {
        const bool has_e = a.E != nullptr, has_gz = a.Gz != nullptr, has_c = a.C != nullptr;
        const long long c0 = (long long)h * a.tile;
        long long oth[U], pe[U];
        float p[U][W], q[U][PASS == kAttnForward ? 1 : W];              // fwd, rows: xsrc[c], V[c]; cols: xdst[r], gn[r]
        float cc[U][kCols ? W : 1];                                      // cols: C[r]
        float ee[U][W], gz[U][PASS == kAttnForward ? 1 : W];
        float v[U][PASS == kAttnForward ? W : 1];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            oth[u] = valid[u] ? ci[e[u]] : 0;
            pe[u] = kCols ? (valid[u] ? perm[e[u]] : 0) : e[u];   // the entry's position in A's arrays
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (kCols) {
                attn_load<T, P>(p[u], a.xdst + oth[u] * a.ld_xdst + c0, n, t, valid[u]);
                attn_load<T, P>(q[u], a.gn + oth[u] * a.ldgn + c0, n, t, valid[u]);
                attn_load<T, P>(cc[u], a.C + oth[u] * a.ldc + c0, n, t, valid[u] && has_c);
            } else {
                attn_load<T, P>(p[u], a.xsrc + oth[u] * a.ld_xsrc + c0, n, t, valid[u]);
                if (PASS == kAttnForward) attn_load<T, P>(v[u], a.V + oth[u] * a.ld_v + c0, n, t, valid[u]);
                else attn_load<T, P>(q[u], a.V + oth[u] * a.ld_v + c0, n, t, valid[u]);
            }
            attn_load<T, P>(ee[u], a.E + pe[u] * a.ld_e + c0, n, t, valid[u] && has_e);
            if (PASS != kAttnForward) attn_load<T, P>(gz[u], a.Gz + pe[u] * a.ldgz + c0, n, t, valid[u] && has_gz);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!valid[u]) continue;
            float z[W];
#pragma unroll
            for (int i = 0; i < W; ++i) z[i] = gate_z(x[i], p[u][i], ee[u][i], has_e);
            if (PASS == kAttnForward) {
                if (a.z) attn_store<T, P>(z, a.z + pe[u] * a.ldz + c0, n, t);
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const float g = gate_sigmoid(z[i]);
                    f[i] = __fmaf_rn(g, v[u][i], f[i]);
                    f[W + i] = __fadd_rn(f[W + i], g);
                }
            } else if (PASS == kAttnBackwardRows) {
                float d[W];
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    d[i] = gate_dz(gate_sigmoid(z[i]), y[i], q[u][i], c[i], gz[u][i], has_gz);
                    f[i] = __fadd_rn(f[i], d[i]);
                }
                if (a.dE) attn_store<T, P>(d, a.dE + pe[u] * a.ld_de + c0, n, t);
            } else {
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const float g = gate_sigmoid(z[i]);
                    f[i] = __fmaf_rn(g, q[u][i], f[i]);
                    f[W + i] = __fadd_rn(f[W + i], gate_dz(g, q[u][i], y[i], cc[u][i], gz[u][i], has_gz));
                }
            }
        }
    }

    static __device__ __forceinline__ void combine(float *g, const float *o) {
#pragma unroll
        for (int i = 0; i < NF; ++i) g[i] = __fadd_rn(g[i], o[i]);
    }

    // cnt: entries of the own row.  An empty row / column: +0 everywhere
    __device__ __forceinline__ void finish(bool writer, int own, int cnt) {
        if (!writer) return;
        const long long r = own, c0 = (long long)h * a.tile;
        if (PASS == kAttnForward) {
            if (a.den) attn_store<T, P>(f + W, a.den + r * a.ldden + c0, n, t);
            if (a.norm) {
#pragma unroll
                for (int i = 0; i < W; ++i) f[i] = cnt > 0 ? __fdiv_rn(f[i], __fadd_rn(f[W + i], a.eps)) : 0.0f;
            }
            attn_store<T, P>(f, a.out + r * a.ldc + c0, n, t);
        } else if (PASS == kAttnBackwardRows) {
            if (a.dxdst) attn_store<T, P>(f, a.dxdst + r * a.ld_dxdst + c0, n, t);
        } else {
            if (a.dV) attn_store<T, P>(f, a.dV + r * a.ld_dv + c0, n, t);
            if (a.dxsrc) attn_store<T, P>(f + W, a.dxsrc + r * a.ld_dxsrc + c0, n, t);
        }
    }
};

}  // namespace sx
