// bf16_convert.h -- bf16 <-> fp32 on bit patterns, for every kernel that keeps fp32 in registers and bf16 in memory: the bf16 SpMM
// (spmm_bf16_kernels.h) and the typed loaders of the pattern passes (pattern_pass.h).  A bf16 value widened to fp32 is the same number
// (16 zero bits appended, no conversion instruction); fp32 -> bf16 rounds once, to nearest even.
#pragma once
#include <hip/hip_runtime.h>

namespace sx {

// fp32 -> bf16 bit pattern, round to nearest even; a NaN stays a (quiet) NaN.  The integer form: the carry of the rounding add runs
// into the exponent, which is what makes the largest finite values round to infinity.
__device__ __forceinline__ unsigned bf16_round(float f) {
    const unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ unsigned bf16_round2(float lo, float hi) { return bf16_round(lo) | (bf16_round(hi) << 16); }
// The same value without a branch: both candidates are computed and one is selected.  For stores inside a loop over gathered entries
// (pattern_pass.h), where the compiler turns bf16_round's early return into a divergent branch per element.
__device__ __forceinline__ unsigned bf16_round_select(float f) {
    const unsigned u = __float_as_uint(f);
    const unsigned quiet = (u >> 16) | 0x40u, even = (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
    return (u & 0x7fffffffu) > 0x7f800000u ? quiet : even;
}
__device__ __forceinline__ unsigned bf16_round2_select(float lo, float hi) { return bf16_round_select(lo) | (bf16_round_select(hi) << 16); }
__device__ __forceinline__ float bf16_lo(unsigned u) { return __uint_as_float(u << 16); }          // the bf16 in bits 0..15, widened
__device__ __forceinline__ float bf16_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }  // the bf16 in bits 16..31

}  // namespace sx
