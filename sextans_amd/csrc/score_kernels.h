// score_kernels.h -- attention over the pattern of a CSR matrix from CALLER-SUPPLIED per-(entry, head) scores, one pass per direction
// (sextans_score_attention_device / sextans_score_attention_backward_device): DGL's edge_softmax + u_mul_e_sum, PyG's softmax(alpha, index)
// + propagate.  The GAT pass of gat_kernels.h with the score READ instead of computed.  No counterpart in the reference.
//
//   SOFTMAX  forward        s_e = S[e, h];  m = max_e s_e;  Z = sum_e exp(s_e - m);  O[r,h,:] = (sum_e exp(s_e - m) V[c,h,:]) / Z;  lse[r,h] = m + log Z
//            backward rows  delta = <O[r,h,:], G[r,h,:]> (registers only);  p = exp(s_e - lse[r,h]);  dS[e,h] = p * (<G[r,h,:], V[c,h,:]> - delta)
//            backward cols  (over A^T)  p = exp(S[perm e, h] - lse[r,h]);  dV[c,h,:] = sum_e p G[r,h,:]
//   WEIGHT   forward        O[r,h,:] = sum_e S[e,h] V[c,h,:]   (FMA, in the slot's entry order)
//            backward rows  dS[e,h] = <G[r,h,:], V[c,h,:]>
//            backward cols  dV[c,h,:] = sum_e S[perm e, h] G[r,h,:]
// fp32 throughout, FMA in the dot products and the V / G accumulations, exp as in the softmax kernels.  From s onward the SOFTMAX forward
// and column pass make GatPass's roundings in GatPass's order (the forward's are HeadSoftmax's, online_softmax.h): fed the scores GAT
// computes, they give its bits (tests/test_score_attention_gpu.py).
//
// S and dS are (nnz, H) row-major in A's entry order, element (e, h) at (long long)e * ld + h, read and written one float at a time (the
// same address in all T lanes of the slot).  The passes plug into the row walking of pattern_pass.h as GatPass does.  The ROW pass has no
// state across slots: an (entry, head) belongs to exactly one slot, whose lane t == 0 stores dS[e, h] -- one plain store per element, no
// read-modify-write, so the heads may sit in the grid (no heads_inside).  The column pass reads S through perm.
#pragma once
#include "attention_kernels.h"

namespace sx {

enum { kScoreSoftmax = 1, kScoreWeight = 2 };   // SEXTANS_SCORE_*

struct ScoreArgs {
    const float *S, *V, *O, *lse, *G;   // read (O, lse: SOFTMAX backward; G: backward)
    float *out, *out_lse, *dS, *dV;     // written
    long long lds, ldv, ldo, ldg, ldds, lddv;
    int H, dv;
};
struct ScoreDropArgs : ScoreArgs { DropArgs drop; };   // attention dropout (SOFTMAX only): the DROP variant of the pass (attention_kernels.h)

// One slot's view of a pass: the interface of AttnPass.
template <int PASS, int MODE, int T_, int P_, int U_, bool DROP = false>
struct ScorePass {
    static_assert(MODE == kScoreSoftmax || !DROP, "the caller holds the weights and can drop them");
    using Args = std::conditional_t<DROP, ScoreDropArgs, ScoreArgs>;
    static constexpr bool kSoft = MODE == kScoreSoftmax;
    static constexpr int T = T_, P = P_, U = U_, W = 4 * P_;
    // forward: (m, Z,) acc; rows: nothing to merge; cols: dV
    static constexpr int NF = PASS == kAttnForward ? (kSoft ? 2 + W : W) : PASS == kAttnBackwardRows ? 1 : W;
    static constexpr bool kMerge = PASS != kAttnBackwardRows;
    const Args &a;
    const int *ci, *perm;
    const int t;
    int h = 0;
    float y[W];   // rows: the own row's G
    float f[NF];
    float lse = 0.f, delta = 0.f;
    uint64_t key = 0;   // DROP: the mask's key

    __device__ __forceinline__ ScorePass(const Args &a_, const int *ci_, const int *perm_, int t_) : a(a_), ci(ci_), perm(perm_), t(t_) {
        if constexpr (DROP) key = drop_key(a.drop);
    }

    __device__ __forceinline__ void begin(bool act, int own_row, int head, bool) {
        h = head;
        const long long r = act ? own_row : 0;
#pragma unroll
        for (int i = 0; i < NF; ++i) f[i] = 0.0f;
        if (PASS == kAttnForward) {
            if (kSoft) f[0] = -INFINITY;   // HeadSoftmax<W>::init's values (online_softmax.h); the call in a branch of its own changes three kernels
        } else if (PASS == kAttnBackwardRows) {
            attn_load<T, P>(y, a.G + r * a.ldg + (long long)h * a.dv, a.dv, t, act);
            if (kSoft) {
                float o[W];
                attn_load<T, P>(o, a.O + r * a.ldo + (long long)h * a.dv, a.dv, t, act);
                delta = attn_dot<T, W>(o, y);
                lse = act ? a.lse[r * a.H + h] : 0.0f;
            }
        }
    }

    __device__ __forceinline__ void batch(const int (&e)[U_], const bool (&valid)[U_]) {
        long long oth[U], pe[U];
        float s[U], p2[U][W], ls[U], mk[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            oth[u] = valid[u] ? ci[e[u]] : 0;
            pe[u] = valid[u] ? (PASS == kAttnBackwardCols ? perm[e[u]] : e[u]) : 0;   // the entry's position in A's arrays
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            s[u] = valid[u] ? a.S[pe[u] * a.lds + h] : 0.0f;
            if (PASS == kAttnBackwardCols) {
                attn_load<T, P>(p2[u], a.G + oth[u] * a.ldg + (long long)h * a.dv, a.dv, t, valid[u]);
                ls[u] = (kSoft && valid[u]) ? a.lse[oth[u] * a.H + h] : 0.0f;
            } else {
                attn_load<T, P>(p2[u], a.V + oth[u] * a.ldv + (long long)h * a.dv, a.dv, t, valid[u]);
                ls[u] = lse;
            }
        }
        if constexpr (DROP) {
#pragma unroll
            for (int u = 0; u < U; ++u) mk[u] = drop_mult(a.drop, key, (int)pe[u], a.H, h);
        }
        if (PASS == kAttnForward && kSoft) {
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
        } else if (PASS == kAttnBackwardRows) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float ds = attn_dot<T, W>(y, p2[u]);
                if (kSoft) {
                    const float p = softmax_exp(__fsub_rn(s[u], ls[u]));
                    if constexpr (DROP) ds = __fmul_rn(mk[u], ds);
                    ds = __fmul_rn(p, __fsub_rn(ds, delta));
                }
                if (valid[u] && t == 0) a.dS[pe[u] * a.ldds + h] = ds;   // this slot alone owns (entry, head)
            }
        } else {   // WEIGHT forward (an invalid entry: s = 0 and a zero row), column pass
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float pm = s[u];
                if (kSoft) {
                    pm = valid[u] ? softmax_exp(__fsub_rn(s[u], ls[u])) : 0.0f;
                    if constexpr (DROP) pm = __fmul_rn(mk[u], pm);
                }
#pragma unroll
                for (int i = 0; i < W; ++i) f[i] = __fmaf_rn(pm, p2[u][i], f[i]);
            }
        }
    }

    // g <- g (+) o: commutative operations only, so both sides of a butterfly exchange compute the same bits
    static __device__ __forceinline__ void combine(float *g, const float *o) {
        if (PASS == kAttnBackwardRows) return;
        if (PASS == kAttnForward && kSoft) {
            HeadSoftmax<W>::combine(g, o);
        } else {
            state_add<NF>(g, o);
        }
    }

    // n: entries of the own row.  An empty row / column: +0 everywhere, lse = -inf
    __device__ __forceinline__ void finish(bool writer, int own_row, int n) {
        if (!writer || PASS == kAttnBackwardRows) return;
        const long long r = own_row;
        if (PASS == kAttnForward && kSoft) {
            const float inv = __fdiv_rn(1.0f, f[1]);
            float o[W];
#pragma unroll
            for (int i = 0; i < W; ++i) o[i] = n > 0 ? __fmul_rn(f[2 + i], inv) : 0.0f;
            attn_store<T, P>(o, a.out + r * a.ldo + (long long)h * a.dv, a.dv, t);
            if (t == 0) a.out_lse[r * a.H + h] = HeadSoftmax<W>::lse(f, n);
        } else if (PASS == kAttnForward) {
            attn_store<T, P>(f, a.out + r * a.ldo + (long long)h * a.dv, a.dv, t);
        } else {
            attn_store<T, P>(f, a.dV + r * a.lddv + (long long)h * a.dv, a.dv, t);
        }
    }
};

}  // namespace sx
