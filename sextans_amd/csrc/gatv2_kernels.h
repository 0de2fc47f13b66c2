// gatv2_kernels.h -- GATv2 graph attention over the pattern of a CSR matrix in one pass per direction
// (sextans_gatv2_attention_device / sextans_gatv2_attention_backward_device): the fused attention of attention_kernels.h with the score
// a . LeakyReLU(x_dst[r] + x_src[c]) -- the activation sits INSIDE the projection, so two scalars per node (gat_kernels.h) cannot
// express it -- and the gathered x_src row as the message.  No counterpart in the reference.
//
//   forward        z_e[k] = x_dst[r,h,k] + x_src[c,h,k];  l_e[k] = z_e[k] > 0 ? z_e[k] : slope * z_e[k];  s_e = <att[h,:], l_e> + bias_e
//                  m = max_e s_e;  Z = sum_e exp(s_e - m);  O[r,h,:] = (sum_e exp(s_e - m) x_src[c,h,:]) / Z;  lse[r,h] = m + log Z
//   backward rows  delta[r,h] = <O[r,h,:], G[r,h,:]>;  p = exp(s_e - lse);  ds = p * (<G[r,h,:], x_src[c,h,:]> - delta)
//                  g_e[k] = ds * (z_e[k] > 0 ? att[h,k] : slope * att[h,k]);  dx_dst[r,h,:] = sum_e g_e
//                  datt_rows[r,h,:] = sum_e ds * l_e;  dbias_e = sum_h ds
//   backward cols  (over A^T)  dx_src[c,h,:] = sum_e (p G[r,h,:] + g_e)   (one accumulator, the p G term first)
//   datt[h,k] = sum_r datt_rows[r,h,k]   (gatv2_datt_chunks, gatv2_datt_total: a two-level sum in a fixed order, below)
// fp32 throughout, FMA in the dot products and the accumulations, exp as in the softmax kernels.  z is ONE rounded add in every pass and
// the add commutes, so the row pass and the column pass see the bits of z the forward saw.  The LeakyReLU is the plain one (a -inf z is
// not special: the mask is the bias, which is added after the dot product).  Nothing of size nnz is written or read besides the bias.
//
// The pass below plugs into the row walking of pattern_pass.h (attn_rows_body, attn_long_body) like GatPass: the same slots of T
// lanes per (row, head), the same groups of E slots per row, the same second walk, long-row workgroups and merges -- so the same fixed
// order of every sum.  An entry costs ONE gathered row in the forward and the row pass (x_src[c]: it is both the score's operand and the
// message) and two in the column pass (x_dst[r], G[r]) plus lse and delta of the other row.  The slot width follows d alone.
#pragma once
#include "attention_kernels.h"

namespace sx {

struct Gatv2Args {
    const float *xdst, *xsrc, *att, *bias, *O, *lse, *G, *delta;   // read (O, lse, G, delta: backward; delta: column pass)
    float *out, *out_lse, *out_delta, *dxdst, *dxsrc, *datt_rows, *dbias;   // written (datt_rows: M x (H d), dense)
    long long ldxd, ldxs, ldo, ldg, lddxd, lddxs;
    int H, d;
    float slope;
};
struct Gatv2DropArgs : Gatv2Args { DropArgs drop; };   // attention dropout: the DROP variant of the pass (attention_kernels.h)

// One slot's view of a pass: the interface of AttnPass / GatPass.
template <int PASS, int T_, int P_, int U_, bool DROP = false>
struct Gatv2Pass {
    using Args = std::conditional_t<DROP, Gatv2DropArgs, Gatv2Args>;
    static constexpr int T = T_, P = P_, U = U_, W = 4 * P_;
    static constexpr int NF = PASS == kAttnForward ? 2 + W : PASS == kAttnBackwardRows ? 2 * W : W;   // forward: m, Z, acc; rows: dx_dst, datt_rows; cols: dx_src
    static constexpr bool kMerge = true;
    const Args &a;
    const int *ci, *perm;
    const int t;
    int h = 0;
    float x[W], w[W], y[W];   // the own row (x_dst; cols: x_src), the head's att, G of the own row (rows pass only)
    float f[NF];
    float lse = 0.f, delta = 0.f;
    uint64_t key = 0;   // DROP: the mask's key

    __device__ __forceinline__ Gatv2Pass(const Args &a_, const int *ci_, const int *perm_, int t_) : a(a_), ci(ci_), perm(perm_), t(t_) {
        if constexpr (DROP) key = drop_key(a.drop);
    }

    __device__ __forceinline__ void begin(bool act, int own_row, int head, bool writer) {
        h = head;
        const long long r = act ? own_row : 0;
        attn_load<T, P>(w, a.att + (long long)h * a.d, a.d, t, true);
        if (PASS == kAttnForward) {
            attn_load<T, P>(x, a.xdst + r * a.ldxd + (long long)h * a.d, a.d, t, act);
            HeadSoftmax<W>::init(f);
        } else if (PASS == kAttnBackwardRows) {
            float o[W];
            attn_load<T, P>(x, a.xdst + r * a.ldxd + (long long)h * a.d, a.d, t, act);
            attn_load<T, P>(y, a.G + r * a.ldg + (long long)h * a.d, a.d, t, act);
            attn_load<T, P>(o, a.O + r * a.ldo + (long long)h * a.d, a.d, t, act);
            delta = attn_dot<T, W>(o, y);
            lse = act ? a.lse[r * a.H + h] : 0.0f;
            if (act && writer && t == 0) a.out_delta[r * a.H + h] = delta;
#pragma unroll
            for (int i = 0; i < NF; ++i) f[i] = 0.0f;
        } else {
            attn_load<T, P>(x, a.xsrc + r * a.ldxs + (long long)h * a.d, a.d, t, act);
#pragma unroll
            for (int i = 0; i < NF; ++i) f[i] = 0.0f;
        }
    }

    __device__ __forceinline__ void batch(const int (&e)[U_], const bool (&valid)[U_]) {
        long long oth[U];
        constexpr int NG = PASS == kAttnBackwardCols ? U : 1;   // the second gathered row exists in the column pass only
        float bs[U], p1[U][W], p2[NG][W], ls[U], dl[U];
#pragma unroll
        for (int u = 0; u < U; ++u) oth[u] = valid[u] ? ci[e[u]] : 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (PASS == kAttnBackwardCols) {
                attn_load<T, P>(p1[u], a.xdst + oth[u] * a.ldxd + (long long)h * a.d, a.d, t, valid[u]);
                attn_load<T, P>(p2[u % NG], a.G + oth[u] * a.ldg + (long long)h * a.d, a.d, t, valid[u]);
                ls[u] = valid[u] ? a.lse[oth[u] * a.H + h] : 0.0f;
                dl[u] = valid[u] ? a.delta[oth[u] * a.H + h] : 0.0f;
                bs[u] = (a.bias && valid[u]) ? a.bias[perm[e[u]]] : 0.0f;
            } else {
                attn_load<T, P>(p1[u], a.xsrc + oth[u] * a.ldxs + (long long)h * a.d, a.d, t, valid[u]);
                ls[u] = lse; dl[u] = delta;
                bs[u] = (a.bias && valid[u]) ? a.bias[e[u]] : 0.0f;
            }
        }
        float mk[U];
        if constexpr (DROP) {
#pragma unroll
            for (int u = 0; u < U; ++u) mk[u] = drop_mult(a.drop, key, valid[u] ? (PASS == kAttnBackwardCols ? perm[e[u]] : e[u]) : 0, a.H, h);
        }
        if (PASS == kAttnForward) {
            float s[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float l[W];
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const float z = __fadd_rn(x[i], p1[u][i]);
                    l[i] = z > 0.0f ? z : __fmul_rn(a.slope, z);
                }
                s[u] = __fadd_rn(attn_dot<T, W>(w, l), bs[u]);
            }
            HeadSoftmax<W>::template absorb<U, DROP>(f, s, valid, mk, p1);
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                // l: the activated sum; c: att times the activation's derivative (z == 0 takes the slope)
                float l[W], c[W];
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const float z = __fadd_rn(p1[u][i], x[i]);   // x_dst + x_src: the add commutes, the bits of the forward
                    l[i] = z > 0.0f ? z : __fmul_rn(a.slope, z);
                    c[i] = z > 0.0f ? w[i] : __fmul_rn(a.slope, w[i]);
                }
                const float s = __fadd_rn(attn_dot<T, W>(w, l), bs[u]);
                const float p = valid[u] ? softmax_exp(__fsub_rn(s, ls[u])) : 0.0f;
                // <G[r], x_src[c]>: rows: G is the own row's, x_src gathered; cols: the other way round
                float dp = PASS == kAttnBackwardCols ? attn_dot<T, W>(p2[u % NG], x) : attn_dot<T, W>(y, p1[u]), pm = p;
                if constexpr (DROP) { dp = __fmul_rn(mk[u], dp); pm = __fmul_rn(mk[u], p); }
                const float ds = valid[u] ? __fmul_rn(p, __fsub_rn(dp, dl[u])) : 0.0f;
                if (PASS == kAttnBackwardCols) {
#pragma unroll
                    for (int i = 0; i < W; ++i) f[i] = __fmaf_rn(ds, c[i], __fmaf_rn(pm, p2[u % NG][i], f[i]));
                } else {
#pragma unroll
                    for (int i = 0; i < W; ++i) {
                        f[i] = __fmaf_rn(ds, c[i], f[i]);
                        f[W + i] = __fmaf_rn(ds, l[i], f[W + i]);
                    }
                    if (a.dbias && valid[u] && t == 0) {
                        // the heads of an entry are taken by this lane one after the other, in ascending order: a plain read-modify-write
                        a.dbias[e[u]] = h == 0 ? ds : __fadd_rn(a.dbias[e[u]], ds);
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
    __device__ __forceinline__ void finish(bool writer, int own_row, int n) {
        if (!writer) return;
        const long long r = own_row;
        if (PASS == kAttnForward) {
            const float inv = __fdiv_rn(1.0f, f[1]);
            float o[W];
#pragma unroll
            for (int i = 0; i < W; ++i) o[i] = n > 0 ? __fmul_rn(f[2 + i], inv) : 0.0f;
            attn_store<T, P>(o, a.out + r * a.ldo + (long long)h * a.d, a.d, t);
            if (t == 0) a.out_lse[r * a.H + h] = HeadSoftmax<W>::lse(f, n);
        } else if (PASS == kAttnBackwardRows) {
            attn_store<T, P>(f, a.dxdst + r * a.lddxd + (long long)h * a.d, a.d, t);
            attn_store<T, P>(f + W, a.datt_rows + (r * a.H + h) * (long long)a.d, a.d, t);
        } else {
            attn_store<T, P>(f, a.dxsrc + r * a.lddxs + (long long)h * a.d, a.d, t);
        }
    }
};

// datt = the sum of datt_rows over ALL rows, in two levels whose order is the definition of datt's bits (no atomics):
//   level 1  part[c, j] = ((+0 + datt_rows[256 c, j]) + datt_rows[256 c + 1, j]) + ..   over the rows of chunk c, ascending
//   level 2  datt[j]    = ((+0 + part[0, j]) + part[1, j]) + ..                          over the chunks, ascending
// j runs over the hd = H d floats of a row.  One workgroup per chunk of kGatv2Chunk rows, thread j (strided when hd > 256) owns a column:
// consecutive threads read consecutive floats of a row.
constexpr int kGatv2Chunk = 256;

__global__ __launch_bounds__(256) void gatv2_datt_chunks(const float *__restrict__ rows, long long M, int hd, float *__restrict__ part) {
    const long long c = blockIdx.x;
    const long long r0 = c * kGatv2Chunk;
    const int n = (int)(M - r0 < kGatv2Chunk ? M - r0 : kGatv2Chunk);
    for (int j = threadIdx.x; j < hd; j += 256) {
        const float *p = rows + r0 * hd + j;
        float s = 0.0f;
        int i = 0;
        for (; i + 8 <= n; i += 8) {   // eight loads in flight, added in ascending order
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = p[(long long)(i + k) * hd];
#pragma unroll
            for (int k = 0; k < 8; ++k) s = __fadd_rn(s, v[k]);
        }
        for (; i < n; ++i) s = __fadd_rn(s, p[(long long)i * hd]);
        part[c * hd + j] = s;
    }
}

__global__ __launch_bounds__(256) void gatv2_datt_total(const float *__restrict__ part, long long nchunks, int hd, float *__restrict__ datt) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= hd) return;
    const float *p = part + j;
    float s = 0.0f;
    long long i = 0;
    for (; i + 8 <= nchunks; i += 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = p[(i + k) * hd];
#pragma unroll
        for (int k = 0; k < 8; ++k) s = __fadd_rn(s, v[k]);
    }
    for (; i < nchunks; ++i) s = __fadd_rn(s, p[i * hd]);
    datt[j] = s;
}

}  // namespace sx
