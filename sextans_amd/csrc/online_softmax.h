// online_softmax.h -- the ONE definition of the running softmax that the softmax families of pattern_pass.h keep in their state f[]:
//   per head     HeadSoftmax<W>     f[0] = m, f[1] = Z, f[2 .. 2 + W) = acc     AttnPassT, GatPass, Gatv2Pass, ScorePass
//   per channel  ChannelSoftmax<W>  m, z, acc, each W floats wide               SoftaggPass, EdgeSoftaggPass, VectorAttnPass
// and what the softmax AGGREGATIONS share beyond the state: SoftaggFrame (begin, score, grad, combine, finish of SoftaggPass and
// EdgeSoftaggPass).  The bit relations between the families hold because each of these lines exists once: a new softmax
// family uses this header and does not copy it.
//
// The state runs on differences to the running maximum only, so a score may be anything finite; the merge of two states takes the larger
// m, rescales both sides and adds -- commutative operations only, so both sides of a butterfly exchange end with the same bits.
//
// Shapes matter.  A __forceinline__ helper is optimised on its own before it is inlined, so it must tell the compiler what the pass's
// own code told it: the state it writes is __restrict__ (it is no alias of the entries' pieces), a value read through a pointer is read
// before the test that masks it, results come per element and not through output arrays, arrays come as plain pointers and not as
// references, and a helper wraps no run of attn_load / attn_store calls.  These are the shapes that left every kernel the instructions it
// had; what could not be shared that way stays inline in its pass and is listed in profiles/online_softmax_device_code.txt.
#pragma once
#include "pattern_pass.h"

namespace sx {

// natural log as the hardware's log2 times ln 2: ONE rounded multiply
__device__ __forceinline__ float softagg_log(float z) { return __fmul_rn(__builtin_amdgcn_logf(z), 0.6931471805599453f); }

template <int W>
struct HeadSoftmax {
    static constexpr int NF = 2 + W;

    static __device__ __forceinline__ void init(float *f) {
        f[0] = -INFINITY;
#pragma unroll
        for (int i = 1; i < NF; ++i) f[i] = 0.0f;
    }

    // U entries: scores s[u], valid[u] = the slot has that entry, value pieces v[u][W]; DROP: the accumulator takes mk[u] p (mk is not
    // read otherwise), m, Z and lse do not see the mask.  One rescale serves the batch.
    template <int U, bool DROP>
    static __device__ __forceinline__ void absorb(float *__restrict__ f, const float *s, const bool *valid, const float *mk, float (*v)[W]) {
        float sm[U], mn = f[0];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float su = s[u];                 // (read before the test: a plain select, no branch around a load)
            sm[u] = valid[u] ? su : -INFINITY;     // (exp gives those +0, and their value pieces are zero)
            mn = fmaxf(mn, sm[u]);                 // (a NaN does not reach m; it reaches Z through its own exp)
        }
        const float mref = mn == -INFINITY ? 0.0f : mn;   // only -inf so far: everything stays +0; a ROW of only -inf ends as 0 / 0
        const float al = softmax_exp(__fsub_rn(f[0], mref));   // 1 when m did not grow
#pragma unroll
        for (int i = 1; i < NF; ++i) f[i] = __fmul_rn(f[i], al);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float p = softmax_exp(__fsub_rn(sm[u], mref));
            f[1] = __fadd_rn(f[1], p);
            float pm = p;
            if constexpr (DROP) pm = __fmul_rn(mk[u], p);
#pragma unroll
            for (int i = 0; i < W; ++i) f[2 + i] = __fmaf_rn(pm, v[u][i], f[2 + i]);
        }
        f[0] = mn;
    }

    // g <- g (+) o
    static __device__ __forceinline__ void combine(float *g, const float *o) {
        const float mn = fmaxf(g[0], o[0]);
        const float mref = mn == -INFINITY ? 0.0f : mn;
        const float ca = softmax_exp(__fsub_rn(g[0], mref)), cb = softmax_exp(__fsub_rn(o[0], mref));
#pragma unroll
        for (int i = 1; i < NF; ++i) g[i] = __fadd_rn(__fmul_rn(g[i], ca), __fmul_rn(o[i], cb));
        g[0] = mn;
    }

    // n: entries of the own row.  An empty row: lse = -inf
    static __device__ __forceinline__ float lse(const float *f, int n) { return n > 0 ? __fadd_rn(f[0], softagg_log(f[1])) : -INFINITY; }
};

// The online softmax of HeadSoftmax per float instead of per head.  A row of one entry ends with z = 1 and acc = the message: the result
// has the message's bits (a -0 message gives +0).
template <int W>
struct ChannelSoftmax {
    static constexpr int NF = 3 * W;

    static __device__ __forceinline__ void init(float *f) {
#pragma unroll
        for (int i = 0; i < W; ++i) {
            f[i] = -INFINITY;
            f[W + i] = 0.0f;
            f[2 * W + i] = 0.0f;
        }
    }

    // U entries: scores s[u][W] (-inf for an entry the slot does not have: exp gives those +0, and their messages are zero), messages m[u][W]
    template <int U>
    static __device__ __forceinline__ void absorb(float *f, float (*s)[W], float (*m)[W]) {
#pragma unroll
        for (int i = 0; i < W; ++i) {
            float mn = f[i];
#pragma unroll
            for (int u = 0; u < U; ++u) mn = fmaxf(mn, s[u][i]);
            const float mref = mn == -INFINITY ? 0.0f : mn;          // only -inf so far: everything stays +0
            const float al = softmax_exp(__fsub_rn(f[i], mref));   // 1 when m did not grow
            float zz = __fmul_rn(f[W + i], al), acc = __fmul_rn(f[2 * W + i], al);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float w = softmax_exp(__fsub_rn(s[u][i], mref));
                zz = __fadd_rn(zz, w);
                acc = __fmaf_rn(w, m[u][i], acc);
            }
            f[i] = mn; f[W + i] = zz; f[2 * W + i] = acc;
        }
    }

    // g <- g (+) o
    static __device__ __forceinline__ void combine(float *g, const float *o) {
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const float mn = fmaxf(g[i], o[i]);
            const float mref = mn == -INFINITY ? 0.0f : mn;
            const float ca = softmax_exp(__fsub_rn(g[i], mref)), cb = softmax_exp(__fsub_rn(o[i], mref));
            g[W + i] = __fadd_rn(__fmul_rn(g[W + i], ca), __fmul_rn(o[W + i], cb));
            g[2 * W + i] = __fadd_rn(__fmul_rn(g[2 * W + i], ca), __fmul_rn(o[2 * W + i], cb));
            g[i] = mn;
        }
    }

    // float i of the results; cnt: entries of the own row.  An empty row: +0 and lse = -inf
    static __device__ __forceinline__ float value(const float *f, int i, int cnt) { return cnt > 0 ? __fdiv_rn(f[2 * W + i], f[W + i]) : 0.0f; }
    static __device__ __forceinline__ float lse(const float *f, int i, int cnt) { return cnt > 0 ? __fadd_rn(f[i], softagg_log(f[W + i])) : -INFINITY; }
};

// g <- g + o: the merge of a state of plain sums
template <int NF>
__device__ __forceinline__ void state_add(float *g, const float *o) {
#pragma unroll
    for (int i = 0; i < NF; ++i) g[i] = __fadd_rn(g[i], o[i]);
}

// A slot's column tile in the per-channel families: COLUMN TILES play the heads' part, a slot of T lanes owns one (row, tile), the last
// tile of a row may be partial.  Tile h starts at column h * a.tile; Args has N and tile.
template <class Args>
__device__ __forceinline__ int tile_floats(const Args &a, int h) { return min(a.tile, a.N - h * a.tile); }   // the tile's valid floats

// What the softmax AGGREGATIONS share (SoftaggPass, EdgeSoftaggPass): one slot's view of a pass, all of it but batch().  The score is the
// message times a temperature per column, the row pass keeps the row's dt sum, the column pass dB.  Args also has t, B, dB, dt_rows.
template <int PASS, class Args_, int T_, int P_>
struct SoftaggFrame {
    using Args = Args_;
    static constexpr int T = T_, P = P_, W = 4 * P_;
    static constexpr int NF = PASS == kAttnForward ? 3 * W : W;   // forward: m, z, acc per float; rows: the dt sum; cols: dB
    static constexpr bool kMerge = true;
    const Args &a;
    const int *ci, *perm;
    const int t;
    int h = 0, n = 0;        // the tile and its valid floats
    float tt[W];             // the tile's temperatures
    float x[W], y[W], z[W];  // backward: the own row's B (cols) or C (rows); rows: the own row's lse and G
    float f[NF];

    __device__ __forceinline__ SoftaggFrame(const Args &a_, const int *ci_, const int *perm_, int t_) : a(a_), ci(ci_), perm(perm_), t(t_) {}

    __device__ __forceinline__ void begin(bool act, int own, int tile, bool) {
        h = tile;
        n = tile_floats(a, h);
        const long long r = act ? own : 0, c0 = (long long)h * a.tile;
        if (a.t) {
            attn_load<T, P>(tt, a.t + c0, n, t, true);
        } else {
#pragma unroll
            for (int i = 0; i < W; ++i) tt[i] = 1.0f;
        }
        if (PASS == kAttnForward) {
            ChannelSoftmax<W>::init(f);
        } else {
            if (PASS == kAttnBackwardRows) {
                attn_load<T, P>(x, a.C + r * a.ldc + c0, n, t, act);
                attn_load<T, P>(y, a.lse + r * a.ldlse + c0, n, t, act);
                attn_load<T, P>(z, a.G + r * a.ldg + c0, n, t, act);
            } else {
                attn_load<T, P>(x, a.B + r * a.ldb + c0, n, t, act);
            }
#pragma unroll
            for (int i = 0; i < NF; ++i) f[i] = 0.0f;
        }
    }

    // s_e from the message: ONE rounded multiply, never fused -- the three passes see the same bits
    __device__ __forceinline__ float score(float m, int i) const { return a.t ? __fmul_rn(tt[i], m) : m; }
    // q_e from the row's C, lse and G at this float: w = exp(s - lse), gw = G w, d = m - C, q = gw fma(t, d, 1)
    __device__ __forceinline__ float grad(float m, float c, float l, float g, int i, float &gw, float &d) const {
        const float w = softmax_exp(__fsub_rn(score(m, i), l));
        d = __fsub_rn(m, c);
        gw = __fmul_rn(g, w);
        return a.t ? __fmul_rn(gw, __fmaf_rn(tt[i], d, 1.0f)) : __fmul_rn(gw, __fadd_rn(d, 1.0f));
    }

    // g <- g (+) o
    static __device__ __forceinline__ void combine(float *g, const float *o) {
        if (PASS == kAttnForward) ChannelSoftmax<W>::combine(g, o);
        else state_add<NF>(g, o);
    }

    // cnt: entries of the own row.  An empty row / column: +0 everywhere, lse = -inf
    __device__ __forceinline__ void finish(bool writer, int own, int cnt) {
        if (!writer) return;
        const long long r = own, c0 = (long long)h * a.tile;
        if (PASS == kAttnForward) {
            float c[W], l[W];
#pragma unroll
            for (int i = 0; i < W; ++i) {
                c[i] = ChannelSoftmax<W>::value(f, i, cnt);
                l[i] = ChannelSoftmax<W>::lse(f, i, cnt);
            }
            attn_store<T, P>(c, a.out + r * a.ldc + c0, n, t);
            if (a.out_lse) attn_store<T, P>(l, a.out_lse + r * a.ldlse + c0, n, t);
        } else if (PASS == kAttnBackwardRows) {
            if (!a.dt_rows) return;
            float d[W];
#pragma unroll
            for (int i = 0; i < W; ++i) d[i] = cnt > 0 ? f[i] : 0.0f;
            attn_store<T, P>(d, a.dt_rows + r * a.N + c0, n, t);
        } else {
            attn_store<T, P>(f, a.dB + r * a.lddb + c0, n, t);
        }
    }
};

}  // namespace sx
