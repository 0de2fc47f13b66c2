// spmm_bf16_kernels.h -- the gather path of the CSR SpMM with bf16 DENSE operands (sextans_spmm_device_rm_bf16): row-major B in bf16,
// row-major C in fp32 or bf16, A's values and every product and sum in fp32.
//
// Why a path of its own: on matrices without B-row reuse the gather kernel is bound by the number of B-row requests, not by bytes
// (DESIGN 9).  A bf16 row of 8 columns is the 16 bytes an fp32 row of 4 columns is, so one request carries twice the columns.
//
// Arithmetic (parity): a bf16 value widened to fp32 is the same number (16 zero bits appended: `u << 16` / `u & 0xffff0000`, no
// conversion instruction), so products, order and rounding are those of spmm_csr_rowgroup<..., RM = true> on the widened B -- one lane
// per output element, a row's products added in ascending CSR order, each product rounded before the add when EXACT -- and the fp32
// result is bit for bit that kernel's.  A bf16 C_in is widened the same way; a bf16 C_out is the fp32 result rounded to nearest even.
#pragma once
#include "bf16_convert.h"   // bf16_round, bf16_round2, bf16_lo, bf16_hi
#include "spmm_csr_kernels.h"

namespace sx {

// Between two rows of a batch: the accumulators are final and the next row is still raw at this point.  Without it the compiler widens
// all four rows of a batch up front (32 registers of widened copies, 72-80 VGPRs, 6-7 waves per SIMD); with it a row is widened just
// before its multiply-adds and the staged kernels fit 64 VGPRs = 8 waves per SIMD, like the fp32 kernel.
#define SX_PIN_ROW(r, b) asm volatile("" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]), "+v"(r[7]), \
                                         "+v"(b.x), "+v"(b.y), "+v"(b.z), "+v"(b.w))
// acc[0..7] += a * (the 8 bf16 of b), widened just before their multiply-adds: a B row in flight costs 4 registers, not 8
template <bool EXACT>
__device__ __forceinline__ void mac8(float (&acc)[8], float a, const uint4 &b) {
    acc[0] = mac<EXACT>(acc[0], a, bf16_lo(b.x)); acc[1] = mac<EXACT>(acc[1], a, bf16_hi(b.x));
    acc[2] = mac<EXACT>(acc[2], a, bf16_lo(b.y)); acc[3] = mac<EXACT>(acc[3], a, bf16_hi(b.y));
    acc[4] = mac<EXACT>(acc[4], a, bf16_lo(b.z)); acc[5] = mac<EXACT>(acc[5], a, bf16_hi(b.z));
    acc[6] = mac<EXACT>(acc[6], a, bf16_lo(b.w)); acc[7] = mac<EXACT>(acc[7], a, bf16_hi(b.w));
}

// ------------------------------------------------------------------------------------------------
// Row-group gather kernel, bf16 B: spmm_csr_rowgroup<LPR, CH, EXACT, STAGE, RM = true> with a lane owning 8 consecutive output columns.
//   LPR lanes per row -> N tile NT = 8 * LPR (64 / 32 / 16 / 8 columns for LPR = 8 / 4 / 2 / 1); one 16-byte load per lane and non-zero.
//   B: the caller's row-major bf16 B at the launch's first column (row c of tile t = the NT values at B + c * ldb + t * NT), addressed
//   with 32-bit byte offsets from a uniform base: K * ldb * 2 < 2^32 (checked by the host; one address register per row in flight).
//   Cin / Cout: row-major at the launch's first column, fp32 (two 16-byte accesses per lane) or, CBF16, bf16 (one); ld in elements.
//   skip (may be null): rows whose C the piece path writes.  Whole-matrix launches only (no row range, no group list: the split form of
//   a mixed plan, which is what the group list of the fp32 kernel serves, is not a native bf16 route).
// ------------------------------------------------------------------------------------------------
// (second launch bound: 8 waves per SIMD asked for on the staged form, which is 2 registers over without it; no scratch either way)
template <int LPR, int CH, bool EXACT, bool STAGE, bool CBF16>
__global__ __launch_bounds__(kBlock, STAGE ? 8 : 1) void spmm_csr_rowgroup_bf16(
    const int *__restrict__ row_ptr, const int *__restrict__ row_end, const int *__restrict__ col_idx, const float *__restrict__ val,
    const uint16_t *__restrict__ B, int64_t ldb, const void *Cin, int64_t ldc_in, void *Cout, int64_t ldc, int M, int ntiles, int nrowblk,
    float alpha, float beta, int use_xcd_remap, const unsigned char *__restrict__ skip) {
    constexpr int NT = 8 * LPR;
    constexpr int RB = kBlock / LPR;
    __shared__ __attribute__((aligned(16))) int smem[STAGE ? CH * 2 : 2];

    const unsigned nwg = (unsigned)nrowblk * (unsigned)ntiles;
    unsigned wg = blockIdx.x;
    if (use_xcd_remap) wg = xcd_remap(wg, nwg);
    const int rowblk = (int)(wg / (unsigned)ntiles);
    const int tile = (int)(wg % (unsigned)ntiles);

    const int tid = threadIdx.x;
    const int slot = tid / LPR;
    const int q = tid % LPR;
    const int row0 = rowblk * RB;
    const int row = row0 + slot;

    // 32-bit byte offsets into B (the host checks K * ldb * 2 < 2^32): a uniform base and one register per B row in flight
    const char *bt = reinterpret_cast<const char *>(B + (int64_t)tile * NT);
    const unsigned ldb2 = (unsigned)ldb * 2u, qoff = 16u * (unsigned)q;
    auto brow = [&](int c) -> const uint4 * { return reinterpret_cast<const uint4 *>(bt + ((unsigned)c * ldb2 + qoff)); };   // my 16 bytes of B row c
    int j = 0, jend = 0;
    const bool mine = row < M && !(skip && skip[row]);
    if (skip && __syncthreads_count(mine) == 0) return;
    if (mine) { j = row_ptr[row]; jend = row_end[row]; }
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // C_in early: in flight under the row loop
    uint4 cw = make_uint4(0u, 0u, 0u, 0u);
    float4 c0 = make_float4(0.f, 0.f, 0.f, 0.f), c1 = c0;
    const int64_t ccol = (int64_t)tile * NT + 8 * q;
    if (mine) {
        if constexpr (CBF16) {
            cw = *reinterpret_cast<const uint4 *>(static_cast<const uint16_t *>(Cin) + (int64_t)row * ldc_in + ccol);
        } else {
            const float4 *p = reinterpret_cast<const float4 *>(static_cast<const float *>(Cin) + (int64_t)row * ldc_in + ccol);
            c0 = p[0]; c1 = p[1];
        }
    }

    if constexpr (STAGE) {
        int2 *s_nz = reinterpret_cast<int2 *>(smem);
        const int bs = row_ptr[row0];
        const int be = row_ptr[min(row0 + RB, M)];
        for (int cs = bs; cs < be; cs += CH) {
            const int n = min(CH, be - cs);
            for (int i = tid; i < n; i += kBlock)
                s_nz[i] = make_int2(col_idx[cs + i], __float_as_int(val[cs + i]));
            __syncthreads();
            const int hi = min(jend, cs + n);
            while (j + 4 <= hi) {
                const int2 e0 = s_nz[j - cs], e1 = s_nz[j - cs + 1], e2 = s_nz[j - cs + 2], e3 = s_nz[j - cs + 3];
                const uint4 b0 = *brow(e0.x);
                uint4 b1 = *brow(e1.x);
                uint4 b2 = *brow(e2.x);
                uint4 b3 = *brow(e3.x);
                mac8<EXACT>(acc, __int_as_float(e0.y), b0); SX_PIN_ROW(acc, b1);
                mac8<EXACT>(acc, __int_as_float(e1.y), b1); SX_PIN_ROW(acc, b2);
                mac8<EXACT>(acc, __int_as_float(e2.y), b2); SX_PIN_ROW(acc, b3);
                mac8<EXACT>(acc, __int_as_float(e3.y), b3);
                j += 4;
            }
            while (j < hi) {
                const int2 e = s_nz[j - cs];
                const uint4 b = *brow(e.x);
                mac8<EXACT>(acc, __int_as_float(e.y), b);
                ++j;
            }
            __syncthreads();
        }
    } else {
        // Direct variant: the LPR lanes of a row fetch LPR consecutive non-zeros with one load each and exchange them with wave
        // shuffles (one lane per row: it walks its row alone, four entries at a time)
        constexpr int U = LPR > 1 ? LPR : 4;
        while (j < jend) {
            const int cnt = min(U, jend - j);
            int c[LPR > 1 ? 1 : U];
            float a[LPR > 1 ? 1 : U];
            if constexpr (LPR > 1) {
                const int me = j + q;
                c[0] = 0; a[0] = 0.f;
                if (me < jend) { c[0] = col_idx[me]; a[0] = val[me]; }
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int i = min(j + u, jend - 1);
                    c[u] = col_idx[i]; a[u] = val[i];
                }
            }
            uint4 b[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int cu = LPR > 1 ? __shfl(c[0], u, LPR) : c[LPR > 1 ? 0 : u];
                b[u] = (u < cnt) ? *brow(cu) : make_uint4(0u, 0u, 0u, 0u);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float au = LPR > 1 ? __shfl(a[0], u, LPR) : a[LPR > 1 ? 0 : u];
                if (u < cnt) mac8<EXACT>(acc, au, b[u]);
            }
            j += U;
        }
    }

    if (!mine) return;
    if constexpr (CBF16) {
        uint4 o;
        o.x = bf16_round2(epilogue<EXACT>(alpha, acc[0], beta, bf16_lo(cw.x)), epilogue<EXACT>(alpha, acc[1], beta, bf16_hi(cw.x)));
        o.y = bf16_round2(epilogue<EXACT>(alpha, acc[2], beta, bf16_lo(cw.y)), epilogue<EXACT>(alpha, acc[3], beta, bf16_hi(cw.y)));
        o.z = bf16_round2(epilogue<EXACT>(alpha, acc[4], beta, bf16_lo(cw.z)), epilogue<EXACT>(alpha, acc[5], beta, bf16_hi(cw.z)));
        o.w = bf16_round2(epilogue<EXACT>(alpha, acc[6], beta, bf16_lo(cw.w)), epilogue<EXACT>(alpha, acc[7], beta, bf16_hi(cw.w)));
        *reinterpret_cast<uint4 *>(static_cast<uint16_t *>(Cout) + (int64_t)row * ldc + ccol) = o;
    } else {
        float4 *p = reinterpret_cast<float4 *>(static_cast<float *>(Cout) + (int64_t)row * ldc + ccol);
        p[0] = make_float4(epilogue<EXACT>(alpha, acc[0], beta, c0.x), epilogue<EXACT>(alpha, acc[1], beta, c0.y),
                           epilogue<EXACT>(alpha, acc[2], beta, c0.z), epilogue<EXACT>(alpha, acc[3], beta, c0.w));
        p[1] = make_float4(epilogue<EXACT>(alpha, acc[4], beta, c1.x), epilogue<EXACT>(alpha, acc[5], beta, c1.y),
                           epilogue<EXACT>(alpha, acc[6], beta, c1.z), epilogue<EXACT>(alpha, acc[7], beta, c1.w));
    }
}

// ------------------------------------------------------------------------------------------------
// Piece kernel, bf16 B: spmm_csr_pieces<LPR, EXACT, RM = true> with 8 columns per lane -- one row group per piece [vbeg[v], vend[v]) of a
// long row, raw fp32 sums into the scratch matrix P (column-major, ldp; no epilogue).  Same pipeline: batches of 8 gathers, the B rows of
// batch k + 1 requested before the multiply-adds of batch k, the entries of batch k + 3 before those of batch k + 1 are used.
// ------------------------------------------------------------------------------------------------
template <int LPR, bool EXACT>
__global__ __launch_bounds__(kBlock) void spmm_csr_pieces_bf16(const int *__restrict__ vbeg, const int *__restrict__ vend,
                                                               const int *__restrict__ col_idx, const float *__restrict__ val,
                                                               const uint16_t *__restrict__ B, int64_t ldb, float *P, int64_t ldp, int v_begin,
                                                               int v_end, int ntiles) {
    constexpr int NT = 8 * LPR;
    constexpr int RB = kBlock / LPR;
    constexpr int E = LPR >= 8 ? 1 : 8 / LPR;   // entries per lane and batch: 8 gathers per batch whatever the tile width
    constexpr int BATCH = E * LPR;
    const int blk = (int)(blockIdx.x / (unsigned)ntiles), tile = (int)(blockIdx.x % (unsigned)ntiles);
    const int tid = threadIdx.x, slot = tid / LPR, q = tid % LPR;
    const int v = v_begin + blk * RB + slot;
    int j = 0, jend = 0;
    if (v < v_end) { j = vbeg[v]; jend = vend[v]; }
    const uint16_t *bq = B + (int64_t)tile * NT + 8 * q;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

    struct Ent { int c[E]; float a[E]; };
    // this lane's E entries of the batch starting at p (clamped inside the piece: never out of bounds; entries past the end are never
    // multiplied)
    auto fetch = [&](int p, Ent &x) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = max(min(p + E * q + e, jend - 1), 0);
            x.c[e] = col_idx[i];
            x.a[e] = val[i];
        }
    };
    auto gather = [&](const Ent &x, uint4 (&b)[BATCH]) {
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            const int cu = __shfl(x.c[u % E], u / E, LPR);   // entry u of the batch sits in lane u / E, slot u % E
            b[u] = *reinterpret_cast<const uint4 *>(bq + (int64_t)cu * ldb);
        }
    };
    auto macs = [&](const Ent &x, const uint4 (&b)[BATCH], int cnt) {
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            const float au = __shfl(x.a[u % E], u / E, LPR);
            if (u < cnt) mac8<EXACT>(acc, au, b[u]);
        }
    };
    if (j < jend) {
        Ent e0, e1, e2, t;
        uint4 bA[BATCH], bB[BATCH];
        fetch(j, e0); fetch(j + BATCH, e1); fetch(j + 2 * BATCH, e2);
        gather(e0, bA);
        int pos = j;
        // entry sets rotate e0 -> e1 -> e2, row sets bA <-> bB: six phases until both are back where they started
        while (pos < jend) {
            gather(e1, bB); fetch(pos + 3 * BATCH, t); macs(e0, bA, jend - pos); e0 = t; pos += BATCH;
            if (pos >= jend) break;
            gather(e2, bA); fetch(pos + 3 * BATCH, t); macs(e1, bB, jend - pos); e1 = t; pos += BATCH;
            if (pos >= jend) break;
            gather(e0, bB); fetch(pos + 3 * BATCH, t); macs(e2, bA, jend - pos); e2 = t; pos += BATCH;
            if (pos >= jend) break;
            gather(e1, bA); fetch(pos + 3 * BATCH, t); macs(e0, bB, jend - pos); e0 = t; pos += BATCH;
            if (pos >= jend) break;
            gather(e2, bB); fetch(pos + 3 * BATCH, t); macs(e1, bA, jend - pos); e1 = t; pos += BATCH;
            if (pos >= jend) break;
            gather(e0, bA); fetch(pos + 3 * BATCH, t); macs(e2, bB, jend - pos); e2 = t; pos += BATCH;
        }
    }
    if (v < v_end) {
        float *o = P + (int64_t)v + (int64_t)(tile * NT + 8 * q) * ldp;
#pragma unroll
        for (int n = 0; n < 8; ++n) o[n * ldp] = acc[n];
    }
}

// fold_hub_pieces for a row-major bf16 C: the pieces of each long row folded in order, epilogue from the widened C_in, result rounded.
// One thread per (row, column).
template <bool EXACT>
__global__ __launch_bounds__(kBlock) void fold_hub_pieces_bf16(const int *__restrict__ vfirst, const int *__restrict__ hub_row,
                                                               const float *__restrict__ P, int64_t ldp, const uint16_t *Cin, int64_t ldc_in,
                                                               uint16_t *Cout, int64_t ldc, int nhub, int N, float alpha, float beta) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (int64_t)nhub * N) return;
    const int k = (int)(t / N), n = (int)(t % N);
    const int v0 = vfirst[k], v1 = vfirst[k + 1];
    float acc = P[(int64_t)v0 + n * ldp];
    for (int v = v0 + 1; v < v1; ++v) acc = acc + P[(int64_t)v + n * ldp];
    const int64_t r = (int64_t)hub_row[k];
    Cout[r * ldc + n] = (uint16_t)bf16_round(epilogue<EXACT>(alpha, acc, beta, bf16_lo((unsigned)Cin[r * ldc_in + n])));
}

// ------------------------------------------------------------------------------------------------
// Converters over a strided row-major matrix (rows x cols, cols % 8 == 0), for the routes that have no bf16 kernel: bf16 -> fp32 is
// exact, fp32 -> bf16 rounds to nearest even.  VEC: 8 elements per thread with 16-byte accesses (both bases 16-byte aligned, bf16 leading
// dimension % 8 == 0, fp32 leading dimension % 4 == 0); otherwise one element per thread with 2- / 4-byte accesses.
// ------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(kBlock) void widen_bf16_matrix(const uint16_t *__restrict__ src, int64_t lds, float *__restrict__ dst, int64_t ldd,
                                                            int64_t rows, int cols) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if constexpr (VEC) {
        const int per = cols / 8;
        if (t >= rows * per) return;
        const int64_t r = t / per;
        const int c = (int)(t % per) * 8;
        const uint4 w = *reinterpret_cast<const uint4 *>(src + r * lds + c);
        float4 *o = reinterpret_cast<float4 *>(dst + r * ldd + c);
        o[0] = make_float4(bf16_lo(w.x), bf16_hi(w.x), bf16_lo(w.y), bf16_hi(w.y));
        o[1] = make_float4(bf16_lo(w.z), bf16_hi(w.z), bf16_lo(w.w), bf16_hi(w.w));
    } else {
        if (t >= rows * cols) return;
        const int64_t r = t / cols;
        const int c = (int)(t % cols);
        dst[r * ldd + c] = bf16_lo((unsigned)src[r * lds + c]);
    }
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void round_bf16_matrix(const float *__restrict__ src, int64_t lds, uint16_t *__restrict__ dst, int64_t ldd,
                                                            int64_t rows, int cols) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if constexpr (VEC) {
        const int per = cols / 8;
        if (t >= rows * per) return;
        const int64_t r = t / per;
        const int c = (int)(t % per) * 8;
        const float4 *p = reinterpret_cast<const float4 *>(src + r * lds + c);
        const float4 a = p[0], b = p[1];
        *reinterpret_cast<uint4 *>(dst + r * ldd + c) =
            make_uint4(bf16_round2(a.x, a.y), bf16_round2(a.z, a.w), bf16_round2(b.x, b.y), bf16_round2(b.z, b.w));
    } else {
        if (t >= rows * cols) return;
        const int64_t r = t / cols;
        const int c = (int)(t % cols);
        dst[r * ldd + c] = (uint16_t)bf16_round(src[r * lds + c]);
    }
}

}  // namespace sx
