// gat_kernels.h -- graph attention (GAT) over the pattern of a CSR matrix in one pass per direction
// (sextans_gat_attention_device / sextans_gat_attention_backward_device): the fused attention of attention_kernels.h with an ADDITIVE
// score and an activation in front of the softmax.  No counterpart in the reference.
//
//   forward        z_e = (adst[r,h] + asrc[c,h]) + bias_e;  s_e = z_e > 0 ? z_e : slope * z_e  (-inf stays -inf);  m = max_e s_e
//                  Z = sum_e exp(s_e - m);  O[r,h,:] = (sum_e exp(s_e - m) V[c,h,:]) / Z;  lse[r,h] = m + log Z
//   backward rows  delta[r,h] = <O[r,h,:], G[r,h,:]>;  p = exp(s_e - lse);  ds = p * (<G[r,h,:], V[c,h,:]> - delta)
//                  dz = z_e > 0 ? ds : slope * ds;  dadst[r,h] = sum_e dz;  dbias_e = sum_h dz
//   backward cols  (over A^T)  dasrc[c,h] = sum_e dz;  dV[c,h,:] = sum_e p G[r,h,:]
// fp32 throughout, FMA in the dot products and the V / G accumulations, exp as in the softmax kernels.  Nothing of size nnz is written or
// read besides the bias.
//
// The pass below plugs into the row walking of pattern_pass.h (attn_rows_body, attn_long_body): the same slots of T lanes per
// (row, head), the same groups of E slots per row, the same second walk, long-row workgroups and merges -- so the same fixed order of
// every sum.  What differs is the entry: it costs ONE 4-byte load (asrc[c,h]; in the column pass adst, lse and delta of the other row,
// the same address in all T lanes of the slot) and one gathered row (V; in the column pass G) -- no K row, no dot product for the score.
// The slot width follows dv alone.  dadst / dasrc are one more float of the slot's partial state f[], identical in the T lanes of a slot
// (every lane adds the same dz), merged by the same butterflies and LDS merge and stored by lane t == 0.
#pragma once
#include "attention_kernels.h"

namespace sx {

struct GatArgs {
    const float *adst, *asrc, *V, *bias, *O, *lse, *G, *delta;   // read (O, lse, G, delta: backward; delta: column pass)
    float *out, *out_lse, *out_delta, *dadst, *dasrc, *dV, *dbias;   // written
    long long ldadst, ldasrc, ldv, ldo, ldg, lddadst, lddasrc, lddv;
    int H, dv;
    float slope;
};
struct GatDropArgs : GatArgs { DropArgs drop; };   // attention dropout: the DROP variant of the pass (attention_kernels.h)

// LeakyReLU that keeps a -inf mask for every slope (0 * -inf would be NaN); NaN stays NaN
__device__ __forceinline__ float gat_act(float z, float slope) { return (z > 0.0f || z == -INFINITY) ? z : __fmul_rn(slope, z); }

// One slot's view of a pass: the interface of AttnPass.
template <int PASS, int T_, int P_, int U_, bool DROP = false>
struct GatPass {
    using Args = std::conditional_t<DROP, GatDropArgs, GatArgs>;
    static constexpr int T = T_, P = P_, U = U_, W = 4 * P_;
    static constexpr int NF = PASS == kAttnForward ? 2 + W : PASS == kAttnBackwardRows ? 1 : 1 + W;   // forward: m, Z, acc; rows: dadst; cols: dasrc, dV
    static constexpr bool kMerge = true;
    const Args &a;
    const int *ci, *perm;
    const int t;
    int h = 0;
    float y[W];   // the own row's vector: G (rows), V (cols)
    float f[NF];
    float own = 0.f, lse = 0.f, delta = 0.f;   // own: adst[r,h] (forward, rows), asrc[c,h] (cols)
    uint64_t key = 0;   // DROP: the mask's key

    __device__ __forceinline__ GatPass(const Args &a_, const int *ci_, const int *perm_, int t_) : a(a_), ci(ci_), perm(perm_), t(t_) {
        if constexpr (DROP) key = drop_key(a.drop);
    }

    __device__ __forceinline__ void begin(bool act, int own_row, int head, bool writer) {
        h = head;
        const long long r = act ? own_row : 0;
        if (PASS == kAttnForward) {
            own = act ? a.adst[r * a.ldadst + h] : 0.0f;
            HeadSoftmax<W>::init(f);
        } else if (PASS == kAttnBackwardRows) {
            float o[W];
            attn_load<T, P>(y, a.G + r * a.ldg + (long long)h * a.dv, a.dv, t, act);
            attn_load<T, P>(o, a.O + r * a.ldo + (long long)h * a.dv, a.dv, t, act);
            delta = attn_dot<T, W>(o, y);
            lse = act ? a.lse[r * a.H + h] : 0.0f;
            own = act ? a.adst[r * a.ldadst + h] : 0.0f;
            if (act && writer && t == 0) a.out_delta[r * a.H + h] = delta;
            f[0] = 0.0f;
        } else {
            own = act ? a.asrc[r * a.ldasrc + h] : 0.0f;
            attn_load<T, P>(y, a.V + r * a.ldv + (long long)h * a.dv, a.dv, t, act);
#pragma unroll
            for (int i = 0; i < NF; ++i) f[i] = 0.0f;
        }
    }

    __device__ __forceinline__ void batch(const int (&e)[U_], const bool (&valid)[U_]) {
        long long oth[U];
        float sc[U], bs[U], p2[U][W], ls[U], dl[U];
#pragma unroll
        for (int u = 0; u < U; ++u) oth[u] = valid[u] ? ci[e[u]] : 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (PASS == kAttnBackwardCols) {
                sc[u] = valid[u] ? a.adst[oth[u] * a.ldadst + h] : 0.0f;
                attn_load<T, P>(p2[u], a.G + oth[u] * a.ldg + (long long)h * a.dv, a.dv, t, valid[u]);
                ls[u] = valid[u] ? a.lse[oth[u] * a.H + h] : 0.0f;
                dl[u] = valid[u] ? a.delta[oth[u] * a.H + h] : 0.0f;
                bs[u] = (a.bias && valid[u]) ? a.bias[perm[e[u]]] : 0.0f;
            } else {
                sc[u] = valid[u] ? a.asrc[oth[u] * a.ldasrc + h] : 0.0f;
                attn_load<T, P>(p2[u], a.V + oth[u] * a.ldv + (long long)h * a.dv, a.dv, t, valid[u]);
                ls[u] = lse; dl[u] = delta;
                bs[u] = (a.bias && valid[u]) ? a.bias[e[u]] : 0.0f;
            }
        }
        float z[U], s[U], mk[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            z[u] = __fadd_rn(__fadd_rn(own, sc[u]), bs[u]);   // (adst + asrc) + bias in every pass: the first add commutes
            s[u] = gat_act(z[u], a.slope);
        }
        if constexpr (DROP) {
#pragma unroll
            for (int u = 0; u < U; ++u) mk[u] = drop_mult(a.drop, key, valid[u] ? (PASS == kAttnBackwardCols ? perm[e[u]] : e[u]) : 0, a.H, h);
        }
        if (PASS == kAttnForward) {
            HeadSoftmax<W>::template absorb<U, DROP>(f, s, valid, mk, p2);
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float p = valid[u] ? softmax_exp(__fsub_rn(s[u], ls[u])) : 0.0f;
                float dp = attn_dot<T, W>(y, p2[u]), pm = p;
                if constexpr (DROP) { dp = __fmul_rn(mk[u], dp); pm = __fmul_rn(mk[u], p); }
                const float ds = valid[u] ? __fmul_rn(p, __fsub_rn(dp, dl[u])) : 0.0f;
                const float dz = z[u] > 0.0f ? ds : __fmul_rn(a.slope, ds);   // (z == 0 takes the slope)
                f[0] = __fadd_rn(f[0], dz);
                if (PASS == kAttnBackwardCols) {
#pragma unroll
                    for (int i = 0; i < W; ++i) f[1 + i] = __fmaf_rn(pm, p2[u][i], f[1 + i]);
                } else if (a.dbias && valid[u] && t == 0) {
                    // the heads of an entry are taken by this lane one after the other, in ascending order: a plain read-modify-write
                    a.dbias[e[u]] = h == 0 ? dz : __fadd_rn(a.dbias[e[u]], dz);
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
    __device__ __forceinline__ void finish(bool writer, int own_row, int n) {
        if (!writer) return;
        const long long r = own_row;
        if (PASS == kAttnForward) {
            const float inv = __fdiv_rn(1.0f, f[1]);
            float o[W];
#pragma unroll
            for (int i = 0; i < W; ++i) o[i] = n > 0 ? __fmul_rn(f[2 + i], inv) : 0.0f;
            attn_store<T, P>(o, a.out + r * a.ldo + (long long)h * a.dv, a.dv, t);
            if (t == 0) a.out_lse[r * a.H + h] = HeadSoftmax<W>::lse(f, n);
        } else if (PASS == kAttnBackwardRows) {
            if (t == 0) a.dadst[r * a.lddadst + h] = f[0];
        } else {
            if (t == 0) a.dasrc[r * a.lddasrc + h] = f[0];
            attn_store<T, P>(f + 1, a.dV + r * a.lddv + (long long)h * a.dv, a.dv, t);
        }
    }
};

}  // namespace sx
