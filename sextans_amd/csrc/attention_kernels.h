// attention_kernels.h -- multi-head attention over the pattern of a CSR matrix in one pass per direction
// (sextans_attention_device / sextans_attention_backward_device).  No counterpart in the reference: its PEs only multiply and accumulate.
//
//   forward        s_e = scale * (<Q[r,h,:], K[c,h,:]> + bias_e);  m = max_e s_e;  Z = sum_e exp(s_e - m)
//                  O[r,h,:] = (sum_e exp(s_e - m) V[c,h,:]) / Z;   lse[r,h] = m + log Z
//   backward rows  delta[r,h] = <O[r,h,:], G[r,h,:]>;  p = exp(s_e - lse);  ds = p * (<G[r,h,:], V[c,h,:]> - delta)
//                  dQ[r,h,:] = sum_e scale ds K[c,h,:];  dbias_e = sum_h scale ds
//   backward cols  (over A^T)  dV[c,h,:] = sum_e p G[r,h,:];  dK[c,h,:] = sum_e scale ds Q[r,h,:]
// fp32 throughout, FMA in the dot products and the accumulations, exp as in the softmax kernels (exp2 of a rounded product).  Nothing of
// size nnz is written or read besides the bias: the forward keeps a running (m, Z, accumulator) per (row, head) and rescales it when m
// grows (online softmax), the backward recomputes p from lse.  NOT bit-equal to the composition sddmm -> row_softmax -> spmm, whose dot
// products round every product and whose sums associate differently; equal within the tolerance of a chain of fp32 operations.
//
// The passes plug into the row walking of pattern_pass.h (slots of T lanes, groups of E slots per row, the second walk, the long-row
// workgroups, the merges).  Both head dimensions share one width 4 T P, the smallest instantiated one (8, 16, 32, 64, 128 floats) that
// holds the larger; pieces beyond d or dv are predicated off.  An entry costs two gathered rows, and one rescale serves a batch of U.
#pragma once
#include <type_traits>

#include "dropout_hash.h"
#include "online_softmax.h"

namespace sx {

struct AttnArgs {
    const float *Q, *K, *V, *bias, *O, *lse, *G, *delta;   // read (O, lse, G, delta: backward; delta: column pass)
    float *out, *out_lse, *out_delta, *dQ, *dK, *dV, *dbias;   // written
    long long ldq, ldk, ldv, ldo, ldg, lddq, lddk, lddv;
    int H, d, dv;
    float scale;
};

// Attention dropout (the *_dropout_device entries; dropout_hash.h): the multiplier m_e,h = 1 / (1 - p) or 0 of (entry, head) is
// recomputed from a hash wherever it is needed.  Scores, m, Z and lse do not see it; the forward's accumulator takes m p, the backward
// applies it to <G, V> and to the p G accumulation.  A COMPILE-TIME variant of the passes (DROP): the kernels without it are the code
// they were before it existed.
struct AttnDropArgs : AttnArgs { DropArgs drop; };

// Edge features (the *_edge_device entries, engine_attention_edge.hip): a key row Ek[e, h, :] and a value row Ev[e, h, :] per stored entry,
// (nnz, H d) and (nnz, H dv) row-major in A's entry order, addressed (long long)e * ld as in spmm_edge_kernels.h:
//   k_e = K[c] + Ek[e],  v_e = V[c] + Ev[e]   (one __fadd_rn per element, formed once per pass), then everything above with k_e, v_e
//   row pass       dEk[e, h, :] = scale ds Q[r, h, :];  dEv[e, h, :] = m p G[r, h, :]   -- an (entry, head) belongs to one slot: plain stores;
//                  dEk == dEv: the sum of the two pieces is stored once
//   column pass    the score and <G[r], v_e> read Ek, Ev a second time, through perm; dK and dV keep their form
// Ek / Ev absent (NULL): a wavefront-uniform test, that side is the plain one.  A COMPILE-TIME variant of the passes (EDGE), as DROP is.
struct AttnEdgeArgs : AttnArgs {
    const float *Ek, *Ev;
    float *dEk, *dEv;   // row pass; NULL: not wanted
    long long ldek, ldev, lddek, lddev;
};
struct AttnEdgeDropArgs : AttnEdgeArgs { DropArgs drop; };

__device__ __forceinline__ uint64_t drop_key(const DropArgs &d) {
    // (volatile: a vector load of the word a captured graph's caller bumps between replays)
    const uint64_t step = d.step ? *reinterpret_cast<const volatile uint64_t *>(d.step) : 0;
    return dropout_key(d.seed, step);
}
// e: the entry's position in the CSR arrays as set (the column pass: perm of the walked position)
__device__ __forceinline__ float drop_mult(const DropArgs &d, uint64_t key, int e, int H, int h) {
    return dropout_u32(key, (uint64_t)e, (uint32_t)H, (uint32_t)h) >= d.thresh ? d.inv_keep : 0.0f;
}

// One slot's view of a pass.  "own" is the row of the pattern walked (a row of A; the column pass: a row of A^T = a column of A),
// "other" the index stored with an entry.
template <int PASS, int T_, int P_, int U_, bool DROP, bool EDGE>
struct AttnPassT {
    using Args = std::conditional_t<EDGE, std::conditional_t<DROP, AttnEdgeDropArgs, AttnEdgeArgs>, std::conditional_t<DROP, AttnDropArgs, AttnArgs>>;
    static constexpr int T = T_, P = P_, U = U_, W = 4 * P_;
    static constexpr int NF = PASS == kAttnForward ? 2 + W : PASS == kAttnBackwardRows ? W : 2 * W;   // forward: m, Z, acc; rows: dQ; cols: dK, dV
    static constexpr bool kMerge = true;
    const Args &a;
    const int *ci, *perm;
    const int t;
    int h = 0;
    float x[W], y[W];   // the own row's vectors: Q (forward), Q and G (rows), K and V (cols)
    float f[NF];
    float lse = 0.f, delta = 0.f;
    uint64_t key = 0;   // DROP: the mask's key

    __device__ __forceinline__ AttnPassT(const Args &a_, const int *ci_, const int *perm_, int t_) : a(a_), ci(ci_), perm(perm_), t(t_) {
        if constexpr (DROP) key = drop_key(a.drop);
    }

    // the slot takes (own, head): `writer` = it is the one slot of its group that stores per-(row, head) results
    __device__ __forceinline__ void begin(bool act, int own, int head, bool writer) {
        h = head;
        const long long r = act ? own : 0;
        if (PASS == kAttnForward) {
            attn_load<T, P>(x, a.Q + r * a.ldq + (long long)h * a.d, a.d, t, act);
            HeadSoftmax<W>::init(f);
        } else if (PASS == kAttnBackwardRows) {
            float o[W];
            attn_load<T, P>(x, a.Q + r * a.ldq + (long long)h * a.d, a.d, t, act);
            attn_load<T, P>(y, a.G + r * a.ldg + (long long)h * a.dv, a.dv, t, act);
            attn_load<T, P>(o, a.O + r * a.ldo + (long long)h * a.dv, a.dv, t, act);
            delta = attn_dot<T, W>(o, y);
            lse = act ? a.lse[r * a.H + h] : 0.0f;
            if (act && writer && t == 0) a.out_delta[r * a.H + h] = delta;
#pragma unroll
            for (int i = 0; i < NF; ++i) f[i] = 0.0f;
        } else {
            attn_load<T, P>(x, a.K + r * a.ldk + (long long)h * a.d, a.d, t, act);
            attn_load<T, P>(y, a.V + r * a.ldv + (long long)h * a.dv, a.dv, t, act);
#pragma unroll
            for (int i = 0; i < NF; ++i) f[i] = 0.0f;
        }
    }

    // U entries of the own row: e[u] their positions in the walked arrays, valid[u] = the slot has that entry
    __device__ __forceinline__ void batch(const int (&e)[U_], const bool (&valid)[U_]) {
        long long oth[U];
        float bs[U], p1[U][W], p2[U][W], ls[U], dl[U];
#pragma unroll
        for (int u = 0; u < U; ++u) oth[u] = valid[u] ? ci[e[u]] : 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (PASS == kAttnBackwardCols) {
                attn_load<T, P>(p1[u], a.Q + oth[u] * a.ldq + (long long)h * a.d, a.d, t, valid[u]);
                attn_load<T, P>(p2[u], a.G + oth[u] * a.ldg + (long long)h * a.dv, a.dv, t, valid[u]);
                ls[u] = valid[u] ? a.lse[oth[u] * a.H + h] : 0.0f;
                dl[u] = valid[u] ? a.delta[oth[u] * a.H + h] : 0.0f;
                bs[u] = (a.bias && valid[u]) ? a.bias[perm[e[u]]] : 0.0f;
            } else {
                attn_load<T, P>(p1[u], a.K + oth[u] * a.ldk + (long long)h * a.d, a.d, t, valid[u]);
                attn_load<T, P>(p2[u], a.V + oth[u] * a.ldv + (long long)h * a.dv, a.dv, t, valid[u]);
                ls[u] = lse; dl[u] = delta;
                bs[u] = (a.bias && valid[u]) ? a.bias[e[u]] : 0.0f;
            }
        }
        long long pe[EDGE ? U : 1];                                  // EDGE: the entry's position in A's arrays
        float ke[EDGE && PASS == kAttnBackwardCols ? U : 1][W];      // EDGE, column pass: k_e (the other passes form it in p1)
        float ve[EDGE && PASS == kAttnBackwardCols ? U : 1][W];
        if constexpr (EDGE) {
            float ek[U][W], ev[U][W];
#pragma unroll
            for (int u = 0; u < U; ++u) pe[u] = PASS == kAttnBackwardCols ? (valid[u] ? perm[e[u]] : 0) : e[u];
            if (a.Ek) {
#pragma unroll
                for (int u = 0; u < U; ++u) attn_load<T, P>(ek[u], a.Ek + pe[u] * a.ldek + (long long)h * a.d, a.d, t, valid[u]);
            }
            if (a.Ev) {
#pragma unroll
                for (int u = 0; u < U; ++u) attn_load<T, P>(ev[u], a.Ev + pe[u] * a.ldev + (long long)h * a.dv, a.dv, t, valid[u]);
            }
            if (PASS == kAttnBackwardCols) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
#pragma unroll
                    for (int i = 0; i < W; ++i) {
                        ke[u][i] = a.Ek ? __fadd_rn(x[i], ek[u][i]) : x[i];
                        ve[u][i] = a.Ev ? __fadd_rn(y[i], ev[u][i]) : y[i];
                    }
                }
            } else {
                if (a.Ek) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
#pragma unroll
                        for (int i = 0; i < W; ++i) p1[u][i] = __fadd_rn(p1[u][i], ek[u][i]);
                    }
                }
                if (a.Ev) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
#pragma unroll
                        for (int i = 0; i < W; ++i) p2[u][i] = __fadd_rn(p2[u][i], ev[u][i]);
                    }
                }
            }
        }
        float s[U], mk[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float dot;
            if constexpr (EDGE && PASS == kAttnBackwardCols) dot = attn_dot<T, W>(ke[u], p1[u]);
            else dot = attn_dot<T, W>(x, p1[u]);
            s[u] = __fmul_rn(a.scale, __fadd_rn(dot, bs[u]));
        }
        if constexpr (DROP) {
#pragma unroll
            for (int u = 0; u < U; ++u) mk[u] = drop_mult(a.drop, key, valid[u] ? (PASS == kAttnBackwardCols ? perm[e[u]] : e[u]) : 0, a.H, h);
        }
        if (PASS == kAttnForward) {
            // HeadSoftmax<W>::absorb (online_softmax.h), kept inline: the call changes this family's wide kernels (profiles/online_softmax_device_code.txt)
            float mn = f[0];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                s[u] = valid[u] ? s[u] : -INFINITY;
                mn = fmaxf(mn, s[u]);
            }
            const float mref = mn == -INFINITY ? 0.0f : mn;
            const float al = softmax_exp(__fsub_rn(f[0], mref));
#pragma unroll
            for (int i = 1; i < NF; ++i) f[i] = __fmul_rn(f[i], al);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float p = softmax_exp(__fsub_rn(s[u], mref));
                f[1] = __fadd_rn(f[1], p);
                float pm = p;
                if constexpr (DROP) pm = __fmul_rn(mk[u], p);
#pragma unroll
                for (int i = 0; i < W; ++i) f[2 + i] = __fmaf_rn(pm, p2[u][i], f[2 + i]);
            }
            f[0] = mn;
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float p = valid[u] ? softmax_exp(__fsub_rn(s[u], ls[u])) : 0.0f;
                float dp, pm = p;
                if constexpr (EDGE && PASS == kAttnBackwardCols) dp = attn_dot<T, W>(ve[u], p2[u]);
                else dp = attn_dot<T, W>(y, p2[u]);
                if constexpr (DROP) { dp = __fmul_rn(mk[u], dp); pm = __fmul_rn(mk[u], p); }
                const float ds = valid[u] ? __fmul_rn(a.scale, __fmul_rn(p, __fsub_rn(dp, dl[u]))) : 0.0f;
#pragma unroll
                for (int i = 0; i < W; ++i) f[i] = __fmaf_rn(ds, p1[u][i], f[i]);
                if (PASS == kAttnBackwardCols) {
#pragma unroll
                    for (int i = 0; i < W; ++i) f[W + i] = __fmaf_rn(pm, p2[u][i], f[W + i]);
                } else if (a.dbias && valid[u] && t == 0) {
                    // the heads of an entry are taken by this lane one after the other, in ascending order: a plain read-modify-write
                    a.dbias[e[u]] = h == 0 ? ds : __fadd_rn(a.dbias[e[u]], ds);
                }
                if constexpr (EDGE && PASS == kAttnBackwardRows) {
                    if (valid[u] && (a.dEk || a.dEv)) {
                        float gk[W], gv[W];
#pragma unroll
                        for (int i = 0; i < W; ++i) {
                            gk[i] = __fmul_rn(ds, x[i]);
                            gv[i] = __fmul_rn(pm, y[i]);
                        }
                        if (a.dEk == a.dEv) {   // one shared gradient (d == dv): the sum, stored once
#pragma unroll
                            for (int i = 0; i < W; ++i) gk[i] = __fadd_rn(gk[i], gv[i]);
                            attn_store<T, P>(gk, a.dEk + pe[u] * a.lddek + (long long)h * a.d, a.d, t);
                        } else {
                            if (a.dEk) attn_store<T, P>(gk, a.dEk + pe[u] * a.lddek + (long long)h * a.d, a.d, t);
                            if (a.dEv) attn_store<T, P>(gv, a.dEv + pe[u] * a.lddev + (long long)h * a.dv, a.dv, t);
                        }
                    }
                }
            }
        }
    }

    // g <- g (+) o: commutative operations only, so both sides of a butterfly exchange compute the same bits
    static __device__ __forceinline__ void combine(float *g, const float *o) {
        if (PASS == kAttnForward) {
            HeadSoftmax<W>::combine(g, o);
        } else {
            state_add<NF>(g, o);
        }
    }

    // n: entries of the own row.  An empty row / column: +0 everywhere, lse = -inf
    __device__ __forceinline__ void finish(bool writer, int own, int n) {
        if (!writer) return;
        const long long r = own;
        if (PASS == kAttnForward) {
            const float inv = __fdiv_rn(1.0f, f[1]);
            float o[W];
#pragma unroll
            for (int i = 0; i < W; ++i) o[i] = n > 0 ? __fmul_rn(f[2 + i], inv) : 0.0f;
            attn_store<T, P>(o, a.out + r * a.ldo + (long long)h * a.dv, a.dv, t);
            if (t == 0) a.out_lse[r * a.H + h] = HeadSoftmax<W>::lse(f, n);
        } else if (PASS == kAttnBackwardRows) {
            attn_store<T, P>(f, a.dQ + r * a.lddq + (long long)h * a.d, a.d, t);
        } else {
            attn_store<T, P>(f, a.dK + r * a.lddk + (long long)h * a.d, a.d, t);
            attn_store<T, P>(f + W, a.dV + r * a.lddv + (long long)h * a.dv, a.dv, t);
        }
    }
};

// The two families' pass types.  AttnPass keeps its own name and parameters: its kernels are the instantiations they were before EDGE existed.
template <int PASS, int T_, int P_, int U_, bool DROP = false>
struct AttnPass : AttnPassT<PASS, T_, P_, U_, DROP, false> {
    using AttnPassT<PASS, T_, P_, U_, DROP, false>::AttnPassT;
};
template <int PASS, int T_, int P_, int U_, bool DROP = false>
struct AttnEdgePass : AttnPassT<PASS, T_, P_, U_, DROP, true> {
    using AttnPassT<PASS, T_, P_, U_, DROP, true>::AttnPassT;
};

}  // namespace sx
