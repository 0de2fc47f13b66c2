// pattern_pass.h -- the row-walking engine under every pass over the pattern of a CSR matrix.  The fourteen families:
//   softmax per head     fused attention and its edge-feature variant (attention_kernels.h), GAT (gat_kernels.h), GATv2 (gatv2_kernels.h),
//                        attention from supplied scores (score_kernels.h)
//   softmax per channel  softmax aggregation (spmm_softagg_kernels.h), of edge messages (spmm_edge_softagg_kernels.h), channel-wise
//                        attention (vector_attention_kernels.h)
//   no softmax           max / min aggregation (spmm_reduce_kernels.h), multi-aggregation (spmm_multi_kernels.h), edge-feature SpMM
//                        (spmm_edge_kernels.h), edge-feature multi-aggregation (spmm_edge_multi_kernels.h), gated aggregation
//                        (spmm_gated_kernels.h), edge-output ops (edge_op_kernels.h)
// The seven softmax families keep their running softmax with the one definition of online_softmax.h.
// A family is a Pass struct (the contract: DESIGN 4.16); this header deals rows to slots, walks their entries, merges the slots' partial
// states and is the ONLY place with a __global__ of this layer: pattern_rows<Pass> and pattern_long<Pass>.
//
// Lanes.  A SLOT of T lanes owns one (row, head) stream of entries: lane t holds the 16-byte pieces t, t + T, .. (P of them) of the
// own row's vectors and of the accumulator, gathers the same pieces of the entries' rows (consecutive lanes, consecutive 16 bytes) and a
// butterfly over the T lanes finishes each dot product.  U entries are in flight per slot: their gathers are issued before the first is
// used.
// Rows.  Dealt by non-zero count with the row softmax's table (wavefront w owns the rows that start in entries [256 w, 256 w + 256)).
// A group of E slots (a power of two, chosen per wavefront so that its rows times heads fill the 64 / T slots) shares a row: slot j takes
// entries j, j + E, .. and the E partial states are merged by a butterfly -- every lane applies the same commutative operations to the
// same pair, so a fixed tree.  A row much longer than its wavefront's mean is taken by all 64 / T slots in a second walk.  Rows beyond
// the softmax's long-row threshold (2048 entries from the row's aligned start) leave the kernel: pattern_long gives each one workgroup
// per head, 256 / T slots striding over the row, merged by the butterfly inside each wavefront and through LDS across the four, in
// wavefront order.  The column pass runs the same code on A^T's arrays and tables.
// Every sum has an order fixed by the pattern and the launch shape: no atomics, the same bits on every run and stream.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>

#include "bf16_convert.h"
#include "row_softmax_common.h"

namespace sx {

enum { kAttnForward = 0, kAttnBackwardRows = 1, kAttnBackwardCols = 2 };

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
// The same pieces of a row that lies in memory as bf16 (16-bit patterns): fp32 in the registers, the same 4 consecutive columns per
// piece -- one 8-byte access -- so a lane holds the columns it holds of an fp32 row.  A read widens exactly, a write rounds once to
// nearest even (bf16_convert.h).  row + col is 8-byte aligned: a 16-byte aligned base, a leading dimension that is a multiple of 4.
template <int T, int P>
__device__ __forceinline__ void attn_load(float *x, const uint16_t *row, int n, int t, bool ok) {
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int col = 4 * (t + T * k);
        uint2 v = make_uint2(0u, 0u);
        if (ok && col < n) v = *reinterpret_cast<const uint2 *>(row + col);
        x[4 * k] = bf16_lo(v.x); x[4 * k + 1] = bf16_hi(v.x); x[4 * k + 2] = bf16_lo(v.y); x[4 * k + 3] = bf16_hi(v.y);
    }
}
template <int T, int P>
__device__ __forceinline__ void attn_store(const float *x, uint16_t *row, int n, int t) {
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const int col = 4 * (t + T * k);
        if (col < n) *reinterpret_cast<uint2 *>(row + col) = make_uint2(bf16_round2_select(x[4 * k], x[4 * k + 1]), bf16_round2_select(x[4 * k + 2], x[4 * k + 3]));
    }
}
template <int T, int W>
__device__ __forceinline__ float attn_dot(const float *x, const float *y) {   // over the slot: every lane ends with the same bits
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < W; ++i) s = __fmaf_rn(x[i], y[i], s);
    return group_sum<T>(s);
}

// entries j, j + E, .. of the n entries that start at b, U at a time (the loop is uniform over the wavefront)
template <class Pass>
__device__ __forceinline__ void walk(Pass &ps, bool act, int b, int n, int j, int E) {
    constexpr int U = Pass::U;
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
        ps.batch(e, valid);
    }
}

// the slot's state with that of the slot `off` lanes away (Pass::kMerge false: the pass keeps no state across slots)
template <class Pass>
__device__ __forceinline__ void merge(Pass &ps, int off) {
    if constexpr (Pass::kMerge) {
        float o[Pass::NF];
#pragma unroll
        for (int i = 0; i < Pass::NF; ++i) o[i] = __shfl_xor(ps.f[i], off);
        Pass::combine(ps.f, o);
    }
}

// The rows [wrow[w], wrow[w + 1]) of wavefront w.  heads_inside: a slot group takes all heads of its row one after the other (the
// row pass with dbias: one lane then owns an entry for every head); otherwise (row, head) pairs are dealt to the groups.
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
            walk(ps, act, b, e - b, j, E);
#pragma unroll 1
            for (int off = T; off < T * E; off <<= 1) merge(ps, off);
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
                walk(ps, true, bb, ee - bb, slot, S);
#pragma unroll 1
                for (int off = T; off < 64; off <<= 1) merge(ps, off);
                ps.finish(slot == 0, r0 + src, ee - bb);
            }
        }
    }
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
        walk(ps, true, b, n, threadIdx.x / T, 256 / T);
#pragma unroll 1
        for (int off = T; off < 64; off <<= 1) merge(ps, off);
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

// The two kernels of every family, pass, width and dropout variant: the Pass type is the whole difference.
template <class Pass>
__global__ __launch_bounds__(256) void pattern_rows(typename Pass::Args a, const int *__restrict__ rp, const int *__restrict__ ci,
                                                    const int *__restrict__ perm, const int *__restrict__ wrow, long long nw, int heads_inside) {
    attn_rows_body<Pass>(a, rp, ci, perm, wrow, nw, heads_inside);
}
template <class Pass>
__global__ __launch_bounds__(256) void pattern_long(typename Pass::Args a, const int *__restrict__ rp, const int *__restrict__ ci,
                                                    const int *__restrict__ perm, const int2 *__restrict__ tab, int heads_inside) {
    attn_long_body<Pass>(a, rp, ci, perm, tab, heads_inside);
}

}  // namespace sx
