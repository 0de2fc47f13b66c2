// sddmm_kernel.h -- sampled dense-dense matmul on the pattern of a CSR matrix, row-major operands (sextans_sddmm_device_rm).
//
// For every stored entry e = (r, c), in CSR order:  acc = +0; acc = acc + X[r, n] * Y[c, n] for n = 0 .. N-1, every product and every
// sum rounded to fp32 (cpu_spmm_CSR's rounding, sparse_helper.h:262-290, applied to a dot product);  out[e] = alpha * acc (+ beta * in[e]).
//
// Work split by NON-ZEROS: wavefront w owns entries [256 w, 256 w + 256), whatever rows they belong to, so a hub row of 10^5 entries is
// spread over hundreds of wavefronts.  A wavefront reads the rows of its first entry and of the next range's first entry from a table built
// once per matrix (sddmm_wave_rows), marks the first entry of every row that starts inside its range and turns the marks
// into a row id per entry with a max-scan; column ids are staged through LDS in one coalesced pass.  Then LPR lanes take one entry, 4
// columns each (a 16-byte gather: at N = 16 the 64-byte Y row is one request), form the products in parallel and pass the running sum
// lane to lane in column order (LPR - 1 moves per 4 * LPR columns).  The X row stays in registers while a lane group's entries stay in
// its row (NCH chunks of 4 * LPR columns; NCH = 0: re-read per entry, for N > 32 * LPR): a group takes every G-th entry of the range, so
// on a mesh row of 81 entries it reads X once per ~5 entries instead of once per entry.  The outputs collect in LDS and leave as 16-byte
// stores.  No atomics.
#pragma once
#include <hip/hip_runtime.h>

namespace sx {

constexpr int kSddmmWaveEntries = 256;

// row0[w] = the row holding entry 256 w (largest r in [0, M) with rp[r] <= 256 w), w < nw; row0[nw] = M - 1.  Once per matrix.
__global__ __launch_bounds__(256) void sddmm_wave_rows(int M, long long nnz, const int *__restrict__ rp, long long nw, int *__restrict__ row0) {
    const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
    if (w > nw) return;
    if (w == nw) { row0[w] = M - 1; return; }
    const long long e = w * kSddmmWaveEntries;
    int lo = 0, hi = M;   // rp[lo] <= e < nnz; the answer lies in [lo, hi)
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (rp[mid] <= e) lo = mid; else hi = mid;
    }
    row0[w] = lo;
}

// one chunk of 4 * LPR columns: rounded products, then the chain of rounded adds through the LPR lanes of the entry in column order
template <int LPR>
__device__ __forceinline__ float sddmm_chunk(float4 x, float4 y, float carry, int sub) {
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

template <int LPR, int NCH>
__global__ __launch_bounds__(256) void sddmm_rowmajor(long long nnz, const int *__restrict__ rp, const int *__restrict__ ci,
                                                      const int *__restrict__ row0, int N, float alpha, const float *__restrict__ X, long long ldx, const float *__restrict__ Y,
                                                      long long ldy, float beta, const float *vin, float *vout) {
    constexpr int G = 64 / LPR;   // entries in flight per wavefront
    __shared__ int s_row[4][kSddmmWaveEntries];
    __shared__ int s_col[4][kSddmmWaveEntries];
    __shared__ float s_out[4][kSddmmWaveEntries];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long e0 = ((long long)blockIdx.x * 4 + wave) * kSddmmWaveEntries;
    const int cnt = e0 < nnz ? (int)min((long long)kSddmmWaveEntries, nnz - e0) : 0;   // (every wavefront reaches every barrier)
    int *srow = s_row[wave], *scol = s_col[wave];
    float *sout = s_out[wave];
    int r_lo = 0, r_hi = -1;   // rows [r_lo, r_hi] cover the range (r_hi: the row of the next range's first entry, or M - 1)
    if (cnt > 0) {
        const long long w = e0 / kSddmmWaveEntries;
        r_lo = row0[w];
        r_hi = row0[w + 1];
    }
    for (int i = lane; i < kSddmmWaveEntries; i += 64) {
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
    const int nch = N / (4 * LPR);
    float4 xc[NCH > 0 ? NCH : 1];   // the X row of the group's current entry (NCH > 0)
    int xrow = -1;
    for (int base = 0; base < cnt; base += G) {
        const int i = base + g;
        const bool act = i < cnt;
        const int r = act ? srow[i] : -1;
        const float *xr = X + (act ? (long long)r * ldx : 0) + 4 * sub;
        const float *yr = Y + (act ? (long long)scol[i] * ldy : 0) + 4 * sub;
        float carry = 0.0f;
        if (NCH > 0) {
            if (act && r != xrow) {
#pragma unroll
                for (int k = 0; k < (NCH > 0 ? NCH : 1); ++k)
                    if (k < nch) xc[k] = *reinterpret_cast<const float4 *>(xr + k * 4 * LPR);
                xrow = r;
            }
#pragma unroll
            for (int k = 0; k < (NCH > 0 ? NCH : 1); ++k) {
                if (k < nch) {
                    float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (act) y = *reinterpret_cast<const float4 *>(yr + k * 4 * LPR);
                    carry = sddmm_chunk<LPR>(xc[k], y, carry, sub);
                }
            }
        } else {
            for (int c0 = 0; c0 < N; c0 += 4 * LPR) {
                float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
                if (act) { x = *reinterpret_cast<const float4 *>(xr + c0); y = *reinterpret_cast<const float4 *>(yr + c0); }
                carry = sddmm_chunk<LPR>(x, y, carry, sub);
            }
        }
        if (act && sub == 0) sout[i] = carry;
    }
    __syncthreads();
    const int i0 = 4 * lane;
    if (i0 < cnt) {
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = __fmul_rn(alpha, sout[i0 + k]);
        if (i0 + 4 <= cnt) {   // 16-byte aligned: e0 is a multiple of 256, the arrays are 16-byte aligned
            if (vin) {
                const float4 v = *reinterpret_cast<const float4 *>(vin + e0 + i0);
                o[0] = __fadd_rn(o[0], __fmul_rn(beta, v.x)); o[1] = __fadd_rn(o[1], __fmul_rn(beta, v.y));
                o[2] = __fadd_rn(o[2], __fmul_rn(beta, v.z)); o[3] = __fadd_rn(o[3], __fmul_rn(beta, v.w));
            }
            *reinterpret_cast<float4 *>(vout + e0 + i0) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
            for (int k = 0; i0 + k < cnt; ++k) {
                float v = o[k];
                if (vin) v = __fadd_rn(v, __fmul_rn(beta, vin[e0 + i0 + k]));
                vout[e0 + i0 + k] = v;
            }
        }
    }
}

}  // namespace sx
