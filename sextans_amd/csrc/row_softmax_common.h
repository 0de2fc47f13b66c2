// row_softmax_common.h -- what the row-softmax kernels (row_softmax_kernels.h) and the fused attention kernels (attention_kernels.h) share:
// the work split's constants, the long-row rule the tables are built by, the lane-group reductions and the exponential.
#pragma once
#include <hip/hip_runtime.h>

namespace sx {

constexpr int kSoftmaxWaveEntries = 256;   // entries a wavefront's rows start in
constexpr int kSoftmaxPieces = 8;          // 16-byte pieces per lane
constexpr int kSoftmaxChunk = 64 * 4 * kSoftmaxPieces;   // 2048: what one wavefront holds; longer rows (counted from their aligned start) take the long-row path

__device__ __forceinline__ int softmax_row_span(int b, int e) { return e - (b & ~3); }   // entries from the row's aligned start to its end

template <int G>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, G));
    return v;
}
template <int G>
__device__ __forceinline__ float group_sum(float v) {   // butterfly: a + b on both sides of every exchange, so every lane ends with the same bits
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v = __fadd_rn(v, __shfl_xor(v, off, G));
    return v;
}

__device__ __forceinline__ float softmax_exp(float d) { return __builtin_amdgcn_exp2f(__fmul_rn(d, 1.4426950408889634f)); }

}  // namespace sx
