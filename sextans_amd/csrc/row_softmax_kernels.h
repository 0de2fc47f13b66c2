// row_softmax_kernels.h -- softmax over the stored entries of every row of a CSR matrix, forward and backward
// (sextans_row_softmax_device / sextans_row_softmax_backward_device).  No counterpart in the reference: its PEs only multiply and accumulate.
//
//   forward    s_e = scale * x_e;  m = max_e s_e;  t_e = exp(s_e - m);  Z = sum_e t_e;  p_e = t_e / Z
//   backward   d = sum_e p_e * g_e;  dx_e = scale * p_e * (g_e - d)
// every product, difference and sum rounded to fp32; exp as exp2 of a rounded product (v_exp_f32); 1 / Z one correctly rounded division
// per row.  The sums are trees: a lane adds at most 32 terms in entry order, a butterfly (__shfl_xor) over the row's lane group adds the
// lanes' sums, and a long row's partial sums are combined the same way -- a fixed association per matrix, no atomics, the same bits on
// every run and stream, and no value passes through more than ~50 consecutive adds.
//
// Work split by NON-ZEROS: wavefront w owns the whole rows whose first entry lies in [256 w, 256 w + 256) (wrow[w] .. wrow[w + 1], a
// table built once per matrix): about 256 entries whatever the row lengths are.  Inside the wavefront a group of G lanes (4 .. 64, from
// the mean row length of the wavefront's rows) takes one row at a time, 64 / G rows side by side.  A lane holds 1 or 2 (whole-wavefront
// rows and long-row chunks: up to 8) aligned 16-byte pieces of its row in registers between the max, the sum and the normalisation: x is
// read once and p written once.  The pieces are
// aligned to 16 bytes in the ARRAY, not in the row: the first and the last piece of a row may reach into its neighbours, whose entries
// are loaded, masked, and never stored (partial pieces are stored entry by entry), which is also what makes the in-place forms safe.
// A row that does not fit its group's registers (more than 4 or 8 G entries) is taken by the whole wavefront in a second walk (up to 2048
// entries).  Longer rows leave the kernel: they are cut into chunks of 2048 entries, one wavefront each (softmax_long_partial writes a
// (max, sum) pair per chunk into a workspace), softmax_long_combine reduces a row's pairs in a fixed order on one wavefront, and
// softmax_long_finish re-reads every chunk and writes it: one more pass over x, for those rows only.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "row_softmax_common.h"

namespace sx {

// wrow[w] = first row r with rp[r] >= 256 w (w < nw), wrow[nw] = M: wavefront w owns rows [wrow[w], wrow[w + 1]).  Once per matrix.
__global__ __launch_bounds__(256) void softmax_wave_rows(int M, const int *__restrict__ rp, long long nw, int *__restrict__ wrow) {
    const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
    if (w > nw) return;
    if (w == nw) { wrow[w] = M; return; }
    const long long e = w * kSoftmaxWaveEntries;
    int lo = 0, hi = M;   // the answer lies in [lo, hi]
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (rp[mid] >= e) hi = mid; else lo = mid + 1;
    }
    wrow[w] = lo;
}

// long rows: cnt[0] += 1, cnt[1] += chunks, per row longer than one wavefront's registers.  Once per matrix (integer atomics: a count)
__global__ __launch_bounds__(256) void softmax_count_long(int M, const int *__restrict__ rp, int *__restrict__ cnt) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= M) return;
    const int b = rp[r], e = rp[r + 1];
    const int span = softmax_row_span(b, e);
    if (e > b && span > kSoftmaxChunk) {
        atomicAdd(&cnt[0], 1);
        atomicAdd(&cnt[1], (span + kSoftmaxChunk - 1) / kSoftmaxChunk);
    }
}

// chunk table: tab[c] = {row, chunk of the row}; a row's chunks are consecutive (where in the table a row lands does not reach any result)
__global__ __launch_bounds__(256) void softmax_fill_long(int M, const int *__restrict__ rp, int *__restrict__ cursor, int nchunks, int2 *__restrict__ tab) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= M) return;
    const int b = rp[r], e = rp[r + 1];
    const int span = softmax_row_span(b, e);
    if (e > b && span > kSoftmaxChunk) {
        const int n = (span + kSoftmaxChunk - 1) / kSoftmaxChunk;
        const int base = atomicAdd(cursor, n);
        for (int i = 0; i < n && base + i < nchunks; ++i) tab[base + i] = make_int2((int)r, i);
    }
}

// The lanes' pieces of one span [a0, a0 + span) of an array (a0 a multiple of 4; entries below `lo` belong to the previous row): piece
// k < NP of lane `sub` of a group of G lanes is entries 4 (sub + G k) .. + 3.  NP is a template parameter chosen per wavefront (group
// walk) or per row (whole-wavefront rows, long-row chunks), so that no piece is loaded, masked or exponentiated that no lane of the
// wavefront can need.  The NP loads are unconditional, from clamped addresses (a piece outside the span reads the array's first piece,
// one cached line for all such lanes): nothing branches around a load, so they issue back to back and are waited for once.
template <int G, int NP>
struct Pieces {
    float4 v[NP];
    __device__ __forceinline__ void load(const float *a, int a0, int span, int nnz, int sub) {
        const int full = nnz & ~3;   // the array's whole 16-byte pieces end here
        if (full > 0) {              // (uniform)
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const int off = 4 * (sub + G * k);
                const int at = (off < span && a0 + off < full) ? a0 + off : 0;
                v[k] = *reinterpret_cast<const float4 *>(a + at);
            }
        } else {
#pragma unroll
            for (int k = 0; k < NP; ++k) v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (a0 + span > full) {   // the matrix's last row reaches the array's last, partial piece: one lane of the whole launch
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const int off = 4 * (sub + G * k);
                if (off < span && a0 + off == full) {
                    v[k].x = a[full];
                    if (full + 1 < nnz) v[k].y = a[full + 1];
                    if (full + 2 < nnz) v[k].z = a[full + 2];
                }
            }
        }
    }
    __device__ __forceinline__ void store(float *a, int a0, int lo, int span, int sub) const {
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int off = 4 * (sub + G * k);
            const int jl = lo - off, jh = span - off;   // entries jl <= j < jh of the piece are the row's
            if (jl <= 0 && jh >= 4) *reinterpret_cast<float4 *>(a + a0 + off) = v[k];
            else if (jh > 0) {
                const float o[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j >= jl && j < jh) a[a0 + off + j] = o[j];
            }
        }
    }
};

// MODE 0: a whole row in one span.  MODE 1: a chunk of a long row, its (max, sum) / partial d to part.  MODE 2: a chunk of a long row
// with the row's max and 1 / Z (forward) or d (backward) given in r0 / r1.  span <= 4 G NP.
template <int G, int NP, bool BWD, int MODE>
__device__ __forceinline__ void softmax_span(int a0, int lo, int span, int nnz, float scale, const float *x, const float *g,
                                             float *out, int sub, float2 *part, float r0, float r1) {
    Pieces<G, NP> X;
    X.load(x, a0, span, nnz, sub);
    if (!BWD) {
        float m = r0, inv = r1;
        // s = scale * x, -inf outside the row (exp gives those +0): the only place the forward masks, so no mask lives across the reductions
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            float *e = &X.v[k].x;
            const int off = 4 * (sub + G * k), jl = lo - off, jh = span - off;   // entries jl <= j < jh of the piece are the row's
#pragma unroll
            for (int j = 0; j < 4; ++j) e[j] = (j >= jl && j < jh) ? __fmul_rn(scale, e[j]) : -INFINITY;
        }
        if (MODE != 2) {
            m = -INFINITY;
#pragma unroll
            for (int k = 0; k < NP; ++k)   // (a NaN does not reach m; it reaches Z through its own t)
                m = fmaxf(fmaxf(m, X.v[k].x), fmaxf(fmaxf(X.v[k].y, X.v[k].z), X.v[k].w));
            m = group_max<G>(m);
        }
        const float mref = (MODE == 1 && m == -INFINITY) ? 0.0f : m;   // a chunk of -inf only adds +0 to its row; a ROW of -inf only is NaN
        float z = 0.0f;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            float *e = &X.v[k].x;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                e[j] = softmax_exp(__fsub_rn(e[j], mref));
                z = __fadd_rn(z, e[j]);
            }
        }
        if (MODE == 1) {
            z = group_sum<G>(z);
            if (sub == 0) *part = make_float2(m, z);
            return;
        }
        if (MODE == 0) inv = __fdiv_rn(1.0f, group_sum<G>(z));
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            X.v[k].x = __fmul_rn(X.v[k].x, inv); X.v[k].y = __fmul_rn(X.v[k].y, inv);
            X.v[k].z = __fmul_rn(X.v[k].z, inv); X.v[k].w = __fmul_rn(X.v[k].w, inv);
        }
        X.store(out, a0, lo, span, sub);
    } else {
        Pieces<G, NP> Gr;
        Gr.load(g, a0, span, nnz, sub);
        float d = r0;
        if (MODE != 2) {
            d = 0.0f;
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const float *p = &X.v[k].x, *q = &Gr.v[k].x;
                const int off = 4 * (sub + G * k), jl = lo - off, jh = span - off;
#pragma unroll
                for (int j = 0; j < 4; ++j) d = __fmaf_rn((j >= jl && j < jh) ? p[j] : 0.0f, (j >= jl && j < jh) ? q[j] : 0.0f, d);
            }
            d = group_sum<G>(d);
        }
        if (MODE == 1) {
            if (sub == 0) *part = make_float2(d, 0.0f);
            return;
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            float *p = &X.v[k].x;
            const float *q = &Gr.v[k].x;
#pragma unroll
            for (int j = 0; j < 4; ++j) p[j] = __fmul_rn(__fmul_rn(scale, p[j]), __fsub_rn(q[j], d));
        }
        X.store(out, a0, lo, span, sub);
    }
}

// one span on all 64 lanes, with as many pieces as it needs (uniform: 256 / 512 / 1024 / 2048 entries)
template <bool BWD, int MODE>
__device__ __forceinline__ void softmax_span64(int a0, int lo, int span, int nnz, float scale, const float *x, const float *g, float *out, int lane,
                                               float2 *part, float r0, float r1) {
    if (span <= 256) softmax_span<64, 1, BWD, MODE>(a0, lo, span, nnz, scale, x, g, out, lane, part, r0, r1);
    else if (span <= 512) softmax_span<64, 2, BWD, MODE>(a0, lo, span, nnz, scale, x, g, out, lane, part, r0, r1);
    else if (span <= 1024) softmax_span<64, 4, BWD, MODE>(a0, lo, span, nnz, scale, x, g, out, lane, part, r0, r1);
    else softmax_span<64, 8, BWD, MODE>(a0, lo, span, nnz, scale, x, g, out, lane, part, r0, r1);
}

// rows [ra, rb) of one wavefront, 64 / G at a time, NP pieces per lane; G = 64: every row through the whole-wavefront form
template <int G, int NP, bool BWD>
__device__ __forceinline__ void softmax_wave(int ra, int rb, int nnz, const int *__restrict__ rp, float scale, const float *x,
                                             const float *g, float *out, int lane) {
    constexpr int RB = 64 / G, CAP = G == 64 ? 0 : 4 * G * NP;
    const int grp = lane / G, sub = lane % G;
    if (G < 64) {
        bool big = false;   // a row too long for its group, short enough for the wavefront
#pragma unroll 1
        for (int r0 = ra; r0 < rb; r0 += RB) {
            const int r = r0 + grp;
            int b = 0, e = 0;
            if (r < rb) { b = rp[r]; e = rp[r + 1]; }
            const int a0 = b & ~3, span = e > b ? e - a0 : 0;
            big |= span > CAP && span <= kSoftmaxChunk;
            if (!__any(span > 0 && span <= CAP)) continue;   // (a batch of empty rows costs its row_ptr reads)
            softmax_span<G, NP, BWD, 0>(a0, b - a0, span <= CAP ? span : 0, nnz, scale, x, g, out, sub, nullptr, 0.f, 0.f);
        }
        if (!__any(big)) return;
    }
    // ... those rows one after the other, all 64 lanes on each (a second walk, so that neither form's registers add to the other's)
#pragma unroll 1
    for (int r0 = ra; r0 < rb; r0 += 64) {
        const int r = r0 + lane;
        int b = 0, e = 0;
        if (r < rb) { b = rp[r]; e = rp[r + 1]; }
        const int span = e > b ? e - (b & ~3) : 0;
        unsigned long long todo = __ballot(span > CAP && span <= kSoftmaxChunk);
#pragma unroll 1
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int bb = __shfl(b, src), ee = __shfl(e, src);
            const int aa = bb & ~3;
            softmax_span64<BWD, 0>(aa, bb - aa, ee - aa, nnz, scale, x, g, out, lane, nullptr, 0.f, 0.f);
        }
    }
}

template <bool BWD>
__global__ __launch_bounds__(256) void row_softmax_rows(int nnz, const int *__restrict__ rp, const int *__restrict__ wrow, long long nw, float scale,
                                                        const float *x, const float *g, float *out) {
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= nw) return;   // (no barrier in this kernel)
    const int ra = wrow[w], rb = wrow[w + 1];
    if (ra >= rb) return;
    // Lane group and pieces per lane from the mean length of the wavefront's rows: q pieces cover a mean row wherever it starts, a
    // quarter more is the headroom; rows beyond it take the whole-wavefront form.  A long row (it leaves the kernel) can only be the
    // last row that starts in the range: it does not count.
    int total = rp[rb] - rp[ra], rows = rb - ra;
    const int last = rp[rb] - rp[rb - 1];
    if (softmax_row_span(rp[rb - 1], rp[rb]) > kSoftmaxChunk && rows > 1) { total -= last; rows -= 1; }
    const int q = (total / rows + 3) / 4 + 1, t = q + q / 4;
    if (t <= 4) softmax_wave<4, 1, BWD>(ra, rb, nnz, rp, scale, x, g, out, lane);
    else if (t <= 8) softmax_wave<4, 2, BWD>(ra, rb, nnz, rp, scale, x, g, out, lane);
    else if (t <= 16) softmax_wave<8, 2, BWD>(ra, rb, nnz, rp, scale, x, g, out, lane);
    else if (t <= 32) softmax_wave<16, 2, BWD>(ra, rb, nnz, rp, scale, x, g, out, lane);
    else if (t <= 64) softmax_wave<32, 2, BWD>(ra, rb, nnz, rp, scale, x, g, out, lane);
    else softmax_wave<64, 1, BWD>(ra, rb, nnz, rp, scale, x, g, out, lane);
}

__device__ __forceinline__ void softmax_chunk_span(const int *__restrict__ rp, int2 rc, int &a0, int &lo, int &span) {
    const int b = rp[rc.x], e = rp[rc.x + 1];
    const int ar = b & ~3;
    a0 = ar + rc.y * kSoftmaxChunk;
    lo = rc.y == 0 ? b - ar : 0;
    span = min(kSoftmaxChunk, e - a0);
}

// one wavefront per chunk of a long row: part[c] = (max, sum of exp(s - max)) of the chunk / (sum of p g, 0)
template <bool BWD>
__global__ __launch_bounds__(256) void softmax_long_partial(int nnz, const int *__restrict__ rp, const int2 *__restrict__ tab, int nchunks, float scale,
                                                            const float *x, const float *g, float2 *__restrict__ part) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= nchunks) return;
    int a0, lo, span;
    softmax_chunk_span(rp, tab[c], a0, lo, span);
    softmax_span64<BWD, 1>(a0, lo, span, nnz, scale, x, g, nullptr, lane, part + c, 0.f, 0.f);
}

// ... then ONE wavefront per long row (the one of its chunk 0) combines the row's pairs in a fixed order -- lane l takes chunks
// l + 64 i in eight interleaved sums (so the longest chain stays at 2048 adds up to 2^20 chunks = 2^31 entries), the eight in order,
// then the butterfly -- and leaves (max, 1 / Z) / (d, 0) in res[first chunk of the row]: linear in the row's length
template <bool BWD>
__global__ __launch_bounds__(256) void softmax_long_combine(const int *__restrict__ rp, const int2 *__restrict__ tab, int nchunks,
                                                            const float2 *__restrict__ part, float2 *__restrict__ res) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= nchunks) return;
    const int2 rc = tab[c];
    if (rc.y != 0) return;
    const int n = (softmax_row_span(rp[rc.x], rp[rc.x + 1]) + kSoftmaxChunk - 1) / kSoftmaxChunk;
    const float2 *pr = part + c;
    float m = -INFINITY;
    if (!BWD) {
        for (int i = lane; i < n; i += 64) m = fmaxf(m, pr[i].x);
        m = group_max<64>(m);
    }
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i0 = lane; i0 < n; i0 += 512) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + 64 * u;
            if (i < n) {
                const float2 q = pr[i];
                // (-inf chunk: 0 * exp(-inf - m) = 0; m = -inf too: NaN, as torch)
                acc[u] = __fadd_rn(acc[u], BWD ? q.x : __fmul_rn(q.y, softmax_exp(__fsub_rn(q.x, m))));
            }
        }
    }
    float z = acc[0];
#pragma unroll
    for (int u = 1; u < 8; ++u) z = __fadd_rn(z, acc[u]);
    z = group_sum<64>(z);
    if (lane == 0) res[c] = BWD ? make_float2(z, 0.0f) : make_float2(m, __fdiv_rn(1.0f, z));
}

// ... and every chunk's wavefront re-reads its chunk and writes it with the row's result
template <bool BWD>
__global__ __launch_bounds__(256) void softmax_long_finish(int nnz, const int *__restrict__ rp, const int2 *__restrict__ tab, int nchunks, float scale,
                                                           const float *x, const float *g, const float2 *__restrict__ res, float *out) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= nchunks) return;
    const int2 rc = tab[c];
    int a0, lo, span;
    softmax_chunk_span(rp, rc, a0, lo, span);
    const float2 r = res[c - rc.y];
    softmax_span64<BWD, 2>(a0, lo, span, nnz, scale, x, g, out, lane, nullptr, r.x, r.y);
}

}  // namespace sx
