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
// Lanes.  A SLOT of T lanes owns one (row, head) stream of entries: lane t holds the 16-byte pieces t, t + T, .. (P of them) of the
// head's Q row and of the accumulator, gathers the same pieces of K[c,h,:] and V[c,h,:] (consecutive lanes, consecutive 16 bytes) and a
// butterfly over the T lanes finishes each dot product.  Both head dimensions share one width 4 T P, the smallest instantiated one
// (8, 16, 32, 64, 128 floats) that holds the larger; pieces beyond d or dv are predicated off.  U entries are in flight per slot: their
// 2 U gathers are issued before the first is used, and one rescale serves the batch.
// Rows.  Dealt by non-zero count with the row softmax's table (wavefront w owns the rows that start in entries [256 w, 256 w + 256)).
// A group of E slots (a power of two, chosen per wavefront so that its rows times heads fill the 64 / T slots) shares a row: slot j takes
// entries j, j + E, .. and the E partial states are merged by a butterfly -- every lane applies the same commutative operations to the
// same pair, so a fixed tree.  A row much longer than its wavefront's mean is taken by all 64 / T slots in a second walk.  Rows beyond
// the softmax's long-row threshold (2048 entries from the row's aligned start) leave the kernel: attn_long gives each one workgroup per
// head, 256 / T slots striding over the row, merged by the butterfly inside each wavefront and through LDS across the four, in
// wavefront order.  The column pass runs the same code on A^T's arrays and tables.
// Every sum has an order fixed by the pattern and the launch shape: no atomics, the same bits on every run and stream.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <type_traits>

#include "dropout_hash.h"
#include "row_softmax_common.h"

namespace sx {

enum { kAttnForward = 0, kAttnBackwardRows = 1, kAttnBackwardCols = 2 };

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

__device__ __forceinline__ uint64_t drop_key(const DropArgs &d) {
    // (volatile: a vector load of the word a captured graph's caller bumps between replays)
    const uint64_t step = d.step ? *reinterpret_cast<const volatile uint64_t *>(d.step) : 0;
    return dropout_key(d.seed, step);
}
// e: the entry's position in the CSR arrays as set (the column pass: perm of the walked position)
__device__ __forceinline__ float drop_mult(const DropArgs &d, uint64_t key, int e, int H, int h) {
    return dropout_u32(key, (uint64_t)e, (uint32_t)H, (uint32_t)h) >= d.thresh ? d.inv_keep : 0.0f;
}

// pieces t, t + T, .. of a row of n floats: x[4 k ..] = row[4 (t + T k) ..], zero beyond n (or when the lane has no row)
template <int T, int P>
__device__ __forceinline__ void attn_load(float *x, const float *row, int n, int t, bool ok) {
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int col = 4 * (t + T * k);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok && col < n) v = *reinterpret_cast<const float4 *>(row + col);
        x[4 * k] = v.x; x[4 * k + 1] = v.y; x[4 * k + 2] = v.z; x[4 * k + 3] = v.w;
    }
}
template <int T, int P>
__device__ __forceinline__ void attn_store(const float *x, float *row, int n, int t) {
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int col = 4 * (t + T * k);
        if (col < n) *reinterpret_cast<float4 *>(row + col) = make_float4(x[4 * k], x[4 * k + 1], x[4 * k + 2], x[4 * k + 3]);
    }
}
template <int T, int W>
__device__ __forceinline__ float attn_dot(const float *x, const float *y) {   // over the slot: every lane ends with the same bits
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < W; ++i) s = __fmaf_rn(x[i], y[i], s);
    return group_sum<T>(s);
}

// One slot's view of a pass.  "own" is the row of the pattern walked (a row of A; the column pass: a row of A^T = a column of A),
// "other" the index stored with an entry.
template <int PASS, int T_, int P_, int U_, bool DROP = false>
struct AttnPass {
    using Args = std::conditional_t<DROP, AttnDropArgs, AttnArgs>;
    static constexpr int T = T_, P = P_, U = U_, W = 4 * P_;
    static constexpr int NF = PASS == kAttnForward ? 2 + W : PASS == kAttnBackwardRows ? W : 2 * W;   // forward: m, Z, acc; rows: dQ; cols: dK, dV
    const Args &a;
    const int *ci, *perm;
    const int t;
    int h = 0;
    float x[W], y[W];   // the own row's vectors: Q (forward), Q and G (rows), K and V (cols)
    float f[NF];
    float lse = 0.f, delta = 0.f;
    uint64_t key = 0;   // DROP: the mask's key

    __device__ __forceinline__ AttnPass(const Args &a_, const int *ci_, const int *perm_, int t_) : a(a_), ci(ci_), perm(perm_), t(t_) {
        if constexpr (DROP) key = drop_key(a.drop);
    }

    // the slot takes (own, head): `writer` = it is the one slot of its group that stores per-(row, head) results
    __device__ __forceinline__ void begin(bool act, int own, int head, bool writer) {
        h = head;
        const long long r = act ? own : 0;
        if (PASS == kAttnForward) {
            attn_load<T, P>(x, a.Q + r * a.ldq + (long long)h * a.d, a.d, t, act);
            f[0] = -INFINITY;
#pragma unroll
            for (int i = 1; i < NF; ++i) f[i] = 0.0f;
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
        float s[U], mk[U];
#pragma unroll
        for (int u = 0; u < U; ++u) s[u] = __fmul_rn(a.scale, __fadd_rn(attn_dot<T, W>(x, p1[u]), bs[u]));
        if constexpr (DROP) {
#pragma unroll
            for (int u = 0; u < U; ++u) mk[u] = drop_mult(a.drop, key, valid[u] ? (PASS == kAttnBackwardCols ? perm[e[u]] : e[u]) : 0, a.H, h);
        }
        if (PASS == kAttnForward) {
            float mn = f[0];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                s[u] = valid[u] ? s[u] : -INFINITY;   // (exp gives those +0, and their V pieces are zero)
                mn = fmaxf(mn, s[u]);                 // (a NaN does not reach m; it reaches Z through its own exp)
            }
            const float mref = mn == -INFINITY ? 0.0f : mn;   // only -inf so far: everything stays +0; a ROW of only -inf ends as 0 / 0
            const float al = softmax_exp(__fsub_rn(f[0], mref));   // 1 when m did not grow
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
                float dp = attn_dot<T, W>(y, p2[u]), pm = p;
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
            }
        }
    }

    // entries j, j + E, .. of the n entries that start at b, U at a time (the loop is uniform over the wavefront)
    __device__ __forceinline__ void walk(bool act, int b, int n, int j, int E) {
        if (!act) n = 0;
#pragma unroll 1
        for (int k0 = j; __any(k0 < n); k0 += E * U) {
            int e[U];
            bool valid[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                valid[u] = k0 + u * E < n;
                e[u] = b + k0 + u * E;
            }
            batch(e, valid);
        }
    }

    // g <- g (+) o: commutative operations only, so both sides of a butterfly exchange compute the same bits
    static __device__ __forceinline__ void combine(float *g, const float *o) {
        if (PASS == kAttnForward) {
            const float mn = fmaxf(g[0], o[0]);
            const float mref = mn == -INFINITY ? 0.0f : mn;
            const float ca = softmax_exp(__fsub_rn(g[0], mref)), cb = softmax_exp(__fsub_rn(o[0], mref));
#pragma unroll
            for (int i = 1; i < NF; ++i) g[i] = __fadd_rn(__fmul_rn(g[i], ca), __fmul_rn(o[i], cb));
            g[0] = mn;
        } else {
#pragma unroll
            for (int i = 0; i < NF; ++i) g[i] = __fadd_rn(g[i], o[i]);
        }
    }
    __device__ __forceinline__ void merge(int off) {   // with the slot `off` lanes away
        float o[NF];
#pragma unroll
        for (int i = 0; i < NF; ++i) o[i] = __shfl_xor(f[i], off);
        combine(f, o);
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
            if (t == 0) a.out_lse[r * a.H + h] = n > 0 ? __fadd_rn(f[0], __fmul_rn(__builtin_amdgcn_logf(f[1]), 0.6931471805599453f)) : -INFINITY;
        } else if (PASS == kAttnBackwardRows) {
            attn_store<T, P>(f, a.dQ + r * a.lddq + (long long)h * a.d, a.d, t);
        } else {
            attn_store<T, P>(f, a.dK + r * a.lddk + (long long)h * a.d, a.d, t);
            attn_store<T, P>(f + W, a.dV + r * a.lddv + (long long)h * a.dv, a.dv, t);
        }
    }
};

// The rows [wrow[w], wrow[w + 1]) of wavefront w.  heads_inside: a slot group takes all heads of its row one after the other (the
// row pass with dbias: one lane then owns an entry for every head); otherwise (row, head) pairs are dealt to the groups.
// (Pass: AttnPass, or the additive-score GatPass of gat_kernels.h -- the row walking does not know how an entry is scored)
template <class Pass>
__device__ __forceinline__ void attn_rows_body(const typename Pass::Args a, const int *__restrict__ rp, const int *__restrict__ ci,
                                               const int *__restrict__ perm, const int *__restrict__ wrow, long long nw, int heads_inside) {
    constexpr int T = Pass::T;
    constexpr int S = 64 / T;   // slots per wavefront
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= nw) return;   // (no barrier in this kernel)
    const int ra = wrow[w], rb = wrow[w + 1];
    if (ra >= rb) return;
    Pass ps(a, ci, perm, lane % T);
    const int slot = lane / T;
    const int HS = heads_inside ? 1 : a.H, nh = heads_inside ? a.H : 1;
    // a long row (it leaves the kernel) can only be the last row that starts in the range: it does not count
    int total = rp[rb] - rp[ra], rows = rb - ra;
    if (softmax_row_span(rp[rb - 1], rp[rb]) > kSoftmaxChunk && rows > 1) { total -= rp[rb] - rp[rb - 1]; rows -= 1; }
    const long long items = (long long)(rb - ra) * HS;
    int E = 1;
    while (2 * E <= S && 2LL * E * items <= S) E *= 2;
    const int cap = E == S ? INT_MAX : E * max(32, 4 * (total / rows));   // longer rows wait for the second walk
    const int per_round = S / E, grp = slot / E, j = slot % E;
    bool big = false;
#pragma unroll 1
    for (long long i0 = 0; i0 < items; i0 += per_round) {
        const long long i = i0 + grp;
        int r = 0, b = 0, e = 0, h0 = 0;
        const bool have = i < items;
        if (have) {
            r = ra + (int)(i / HS);
            h0 = (int)(i % HS);
            b = rp[r]; e = rp[r + 1];
        }
        const bool is_long = e > b && softmax_row_span(b, e) > kSoftmaxChunk;
        const bool is_big = have && !is_long && e - b > cap;
        big |= is_big;
        const bool act = have && !is_long && !is_big;
        if (!__any(act)) continue;
#pragma unroll 1
        for (int hh = 0; hh < nh; ++hh) {
            ps.begin(act, r, h0 + hh, j == 0);
            ps.walk(act, b, e - b, j, E);
#pragma unroll 1
            for (int off = T; off < T * E; off <<= 1) ps.merge(off);
            ps.finish(act && j == 0, r, e - b);
        }
    }
    if (!__any(big)) return;
    // ... those rows one after the other, all slots on each
#pragma unroll 1
    for (int r0 = ra; r0 < rb; r0 += 64) {
        const int r = r0 + lane;
        int b = 0, e = 0;
        if (r < rb) { b = rp[r]; e = rp[r + 1]; }
        unsigned long long todo = __ballot(e - b > cap && softmax_row_span(b, e) <= kSoftmaxChunk);
#pragma unroll 1
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int bb = __shfl(b, src), ee = __shfl(e, src);
#pragma unroll 1
            for (int hh = 0; hh < a.H; ++hh) {
                ps.begin(true, r0 + src, hh, slot == 0);
                ps.walk(true, bb, ee - bb, slot, S);
#pragma unroll 1
                for (int off = T; off < 64; off <<= 1) ps.merge(off);
                ps.finish(slot == 0, r0 + src, ee - bb);
            }
        }
    }
}

template <int PASS, int T, int P, int U>
__global__ __launch_bounds__(256) void attn_rows(AttnArgs a, const int *__restrict__ rp, const int *__restrict__ ci, const int *__restrict__ perm,
                                                 const int *__restrict__ wrow, long long nw, int heads_inside) {
    attn_rows_body<AttnPass<PASS, T, P, U>>(a, rp, ci, perm, wrow, nw, heads_inside);
}

// One workgroup per long row (the workgroup of its chunk 0 in the softmax's chunk table) and head -- heads_inside: per long row, the
// heads one after the other.  The four wavefronts' states meet in LDS and are merged by the first slot in wavefront order.
template <class Pass>
__device__ __forceinline__ void attn_long_body(const typename Pass::Args a, const int *__restrict__ rp, const int *__restrict__ ci,
                                               const int *__restrict__ perm, const int2 *__restrict__ tab, int heads_inside) {
    constexpr int T = Pass::T;
    __shared__ float s_f[4][Pass::NF][T];
    const int2 rc = tab[blockIdx.x];
    if (rc.y != 0) return;   // (uniform: before every barrier)
    const int r = rc.x, b = rp[r], n = rp[r + 1] - b;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, t = lane % T;
    const bool first = threadIdx.x < T;
    Pass ps(a, ci, perm, t);
    const int h0 = heads_inside ? 0 : (int)blockIdx.y, nh = heads_inside ? a.H : 1;
#pragma unroll 1
    for (int hh = 0; hh < nh; ++hh) {
        ps.begin(true, r, h0 + hh, first);
        ps.walk(true, b, n, threadIdx.x / T, 256 / T);
#pragma unroll 1
        for (int off = T; off < 64; off <<= 1) ps.merge(off);
        if (lane < T && wave > 0) {
#pragma unroll
            for (int i = 0; i < Pass::NF; ++i) s_f[wave][i][t] = ps.f[i];
        }
        __syncthreads();
        if (first) {
#pragma unroll 1
            for (int w = 1; w < 4; ++w) {
                float o[Pass::NF];
#pragma unroll
                for (int i = 0; i < Pass::NF; ++i) o[i] = s_f[w][i][t];
                Pass::combine(ps.f, o);
            }
        }
        ps.finish(first, r, n);
        __syncthreads();   // (s_f is written again for the next head)
    }
}

template <int PASS, int T, int P, int U>
__global__ __launch_bounds__(256) void attn_long(AttnArgs a, const int *__restrict__ rp, const int *__restrict__ ci, const int *__restrict__ perm,
                                                 const int2 *__restrict__ tab, int heads_inside) {
    attn_long_body<AttnPass<PASS, T, P, U>>(a, rp, ci, perm, tab, heads_inside);
}

// the same two kernels with the dropout mask (launched only when p > 0)
template <int PASS, int T, int P, int U>
__global__ __launch_bounds__(256) void attn_rows_drop(AttnDropArgs a, const int *__restrict__ rp, const int *__restrict__ ci,
                                                      const int *__restrict__ perm, const int *__restrict__ wrow, long long nw, int heads_inside) {
    attn_rows_body<AttnPass<PASS, T, P, U, true>>(a, rp, ci, perm, wrow, nw, heads_inside);
}
template <int PASS, int T, int P, int U>
__global__ __launch_bounds__(256) void attn_long_drop(AttnDropArgs a, const int *__restrict__ rp, const int *__restrict__ ci,
                                                      const int *__restrict__ perm, const int2 *__restrict__ tab, int heads_inside) {
    attn_long_body<AttnPass<PASS, T, P, U, true>>(a, rp, ci, perm, tab, heads_inside);
}

}  // namespace sx
