// edge_dot_kernels.h -- the per-head dot product of both endpoints of every stored entry of a CSR pattern, row-major operands
// (sextans_edge_dot_device): DGL's u_dot_v, the producer of the (nnz, H) scores that score_kernels.h, gat_kernels.h and gatv2_kernels.h
// read.  No counterpart in the reference.
//
// For every stored entry e = (r, c), in CSR order, and every head h:  acc = +0; acc = acc + X[r, h, n] * Y[c, h, n] for n = 0 .. d-1,
// every product and every sum rounded to fp32, no FMA;  S[e, h] = acc -- sddmm_kernel.h's rounding on the head's slice, bit for bit.
//
// Work split by NON-ZEROS on sddmm_kernel.h's scheme: wavefront w owns entries [256 w, 256 w + 256), reads the rows of its first entry
// and of the next range's first entry from the engine's d_sddmm_row0, marks the first entry of every row that starts inside its range,
// turns the marks into a row id per entry with a max-scan and stages the column ids through LDS -- ONCE for all heads.  The unit of work
// after that is the PAIR p = i * H + h of the range's entry i and head h, i.e. (entry, head) is the virtual entry of an SDDMM with N = d:
// LPR lanes take one pair, 4 columns each (16-byte gathers), form the products in parallel and pass the running sum lane to lane in
// column order.  The 64 / LPR pairs in flight are consecutive, so the lane groups of one load instruction read the neighbouring heads of
// one Y row (at d = 16, H = 8 the 16 groups of an instruction read the whole 512-byte Y rows of two entries) -- the pieces of a Y row
// are gathered together and every entry's column id, row id and row-table words are read once.  A group steps by 64 / LPR pairs: when
// H divides that, it keeps its head and the X piece X[r, h, :] stays in registers while its entries stay in row r (NCH chunks of
// 4 * LPR columns, as sddmm_rowmajor; NCH = 0: re-read per pair); otherwise the piece changes with every step and is re-read (the compare
// is all the reuse costs).  Pairs leave in rounds of 256: with lds == H the pairs of a wavefront are one contiguous run of 256 H floats
// of S, so a round collects in LDS and leaves as one 16-byte store per lane; with lds > H every pair is a plain store by its first lane.
// No atomics.
#pragma once
#include <hip/hip_runtime.h>

namespace sx {

constexpr int kEdgeDotWaveEntries = 256;   // the ranges of the engine's d_sddmm_row0 (sddmm_kernel.h's kSddmmWaveEntries)

// one chunk of 4 * LPR columns: rounded products, then the chain of rounded adds through the LPR lanes of the pair in column order
// (sddmm_chunk's operations in sddmm_chunk's order)
template <int LPR>
__device__ __forceinline__ float edge_dot_chunk(float4 x, float4 y, float carry, int sub) {
    const float p0 = __fmul_rn(x.x, y.x), p1 = __fmul_rn(x.y, y.y), p2 = __fmul_rn(x.z, y.z), p3 = __fmul_rn(x.w, y.w);
    float acc = carry;
#pragma unroll
    for (int j = 0; j < LPR; ++j) {
        if (sub == j) acc = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(acc, p0), p1), p2), p3);
        if (j + 1 < LPR) {
            const float t = __shfl_up(acc, 1, LPR);
            if (sub == j + 1) acc = t;
        }
    }
    return __shfl(acc, LPR - 1, LPR);
}

// H >= 1 heads of d columns, d a multiple of 4 * LPR; X has ldx >= H d, Y ldy >= H d; S is (nnz, H) at lds >= H
template <int LPR, int NCH>
__global__ __launch_bounds__(256) void edge_dot_forward(long long nnz, const int *__restrict__ rp, const int *__restrict__ ci,
                                                        const int *__restrict__ row0, int H, int d, const float *__restrict__ X, long long ldx,
                                                        const float *__restrict__ Y, long long ldy, float *__restrict__ S, long long lds) {
    constexpr int G = 64 / LPR;   // pairs in flight per wavefront
    constexpr int kRound = kEdgeDotWaveEntries;   // pairs per round
    __shared__ int s_row[4][kEdgeDotWaveEntries];
    __shared__ int s_col[4][kEdgeDotWaveEntries];
    __shared__ float s_out[4][kRound];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long e0 = ((long long)blockIdx.x * 4 + wave) * kEdgeDotWaveEntries;
    const int cnt = e0 < nnz ? (int)min((long long)kEdgeDotWaveEntries, nnz - e0) : 0;   // (every wavefront reaches every barrier)
    int *srow = s_row[wave], *scol = s_col[wave];
    float *sout = s_out[wave];
    int r_lo = 0, r_hi = -1;   // rows [r_lo, r_hi] cover the range (r_hi: the row of the next range's first entry, or M - 1)
    if (cnt > 0) {
        const long long w = e0 / kEdgeDotWaveEntries;
        r_lo = row0[w];
        r_hi = row0[w + 1];
    }
    for (int i = lane; i < kEdgeDotWaveEntries; i += 64) {
        srow[i] = i == 0 ? r_lo : -1;
        scol[i] = i < cnt ? ci[e0 + i] : 0;
    }
    __syncthreads();
    for (int r = r_lo + 1 + lane; r <= r_hi; r += 64) {   // first entry of every non-empty row that starts inside the range
        const int b = rp[r];
        if (b < rp[r + 1] && b - e0 < cnt) srow[b - e0] = r;
    }
    __syncthreads();
    {   // max-scan: row id of every entry (lane l holds slots 4 l .. 4 l + 3)
        const int v0 = srow[4 * lane], v1 = max(v0, srow[4 * lane + 1]), v2 = max(v1, srow[4 * lane + 2]), v3 = max(v2, srow[4 * lane + 3]);
        int incl = v3;
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off);
            if (lane >= off) incl = max(incl, t);
        }
        int excl = __shfl_up(incl, 1);
        if (lane == 0) excl = -1;
        srow[4 * lane] = max(excl, v0); srow[4 * lane + 1] = max(excl, v1); srow[4 * lane + 2] = max(excl, v2); srow[4 * lane + 3] = max(excl, v3);
    }
    __syncthreads();
    const int g = lane / LPR, sub = lane % LPR;
    const int nch = d / (4 * LPR);
    const int npairs = cnt * H;        // pair p = i * H + h of the range: S[(e0 + i) * lds + h]
    const bool packed = lds == H;      // (the same in every wavefront: the barriers below are uniform)
    const int step_i = G / H, step_h = G % H;
    int i = g / H, hd = g % H;         // the group's pair, advanced by G pairs per step without a division
    float *Sw = S + e0 * lds;
    float4 xc[NCH > 0 ? NCH : 1];      // the X piece of the group's current (row, head) (NCH > 0)
    long long xat = -1;
    for (int q0 = 0; q0 < kRound * H; q0 += kRound) {   // H rounds in every wavefront, the ones past npairs idle
        if (q0 < npairs) {
#pragma unroll 1
            for (int b = g; b < kRound; b += G) {
                const bool act = q0 + b < npairs;
                const long long xo = act ? (long long)srow[i] * ldx + (long long)hd * d : 0;
                const float *xr = X + xo + 4 * sub;
                const float *yr = Y + (act ? (long long)scol[i] * ldy + (long long)hd * d : 0) + 4 * sub;
                float carry = 0.0f;
                if (NCH > 0) {
                    if (act && xo != xat) {
#pragma unroll
                        for (int k = 0; k < (NCH > 0 ? NCH : 1); ++k)
                            if (k < nch) xc[k] = *reinterpret_cast<const float4 *>(xr + k * 4 * LPR);
                        xat = xo;
                    }
#pragma unroll
                    for (int k = 0; k < (NCH > 0 ? NCH : 1); ++k) {
                        if (k < nch) {
                            float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
                            if (act) y = *reinterpret_cast<const float4 *>(yr + k * 4 * LPR);
                            carry = edge_dot_chunk<LPR>(xc[k], y, carry, sub);
                        }
                    }
                } else {
                    for (int c0 = 0; c0 < d; c0 += 4 * LPR) {
                        float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
                        if (act) { x = *reinterpret_cast<const float4 *>(xr + c0); y = *reinterpret_cast<const float4 *>(yr + c0); }
                        carry = edge_dot_chunk<LPR>(x, y, carry, sub);
                    }
                }
                if (act && sub == 0) {
                    if (packed) sout[b] = carry;
                    else Sw[(long long)i * lds + hd] = carry;
                }
                i += step_i;
                hd += step_h;
                if (hd >= H) { hd -= H; ++i; }
            }
        }
        if (packed) {
            __syncthreads();
            const int p0 = q0 + 4 * lane;
            if (p0 + 4 <= npairs) {   // 16-byte aligned: e0 H and q0 are multiples of 256, S is 16-byte aligned
                *reinterpret_cast<float4 *>(Sw + p0) = make_float4(sout[4 * lane], sout[4 * lane + 1], sout[4 * lane + 2], sout[4 * lane + 3]);
            } else {
                for (int k = 0; p0 + k < npairs; ++k) Sw[p0 + k] = sout[4 * lane + k];
            }
            __syncthreads();
        }
    }
}

}  // namespace sx
