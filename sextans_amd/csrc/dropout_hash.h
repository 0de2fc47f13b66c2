// dropout_hash.h -- the attention-dropout mask (include/sextans_amd.h, sextans_dropout): a counter-based generator, so the forward, the
// row pass over A and the column pass over A^T recompute the same mask from (seed, step, entry, head) alone -- no state of size nnz, no
// atomics, the same bits on every run.  ONE definition for the host (sextans_dropout_keep_host) and the device.
//
//   mix(x)   the SplitMix64 finaliser of x + 0x9E3779B97F4A7C15 (uint64, wrapping)
//   key    = mix(seed + step)                            once per call (per thread on the device)
//   u      = (uint32)(mix(key + e * heads + h) >> 32)    e: the entry's position in the CSR arrays as set, h: the head
//   keep   = u >= thresh,  thresh = (uint32)((double)p * 2^32)   (p in [0, 1); p == 0: thresh == 0, everything is kept)
//   mult   = keep ? 1.0f / (1.0f - p) : 0.0f             (two rounded fp32 operations, made once on the host)
// No counterpart in the reference.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SX_HOST_DEVICE __host__ __device__
#else
#define SX_HOST_DEVICE
#endif

namespace sx {

SX_HOST_DEVICE inline uint64_t dropout_mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

SX_HOST_DEVICE inline uint64_t dropout_key(uint64_t seed, uint64_t step) { return dropout_mix(seed + step); }

// the 32 bits compared with thresh; e: entry, h: head
SX_HOST_DEVICE inline uint32_t dropout_u32(uint64_t key, uint64_t e, uint32_t heads, uint32_t h) {
    return (uint32_t)(dropout_mix(key + e * heads + h) >> 32);
}

inline uint32_t dropout_thresh(float p) { return (uint32_t)((double)p * 4294967296.0); }
inline float dropout_scale(float p) { return 1.0f / (1.0f - p); }

// what a kernel gets (by value, behind its other arguments)
struct DropArgs {
    uint64_t seed;
    const uint64_t *step;   // NULL: step 0; else one device word, read once per thread
    uint32_t thresh;        // keep when u >= thresh
    float inv_keep;         // 1 / (1 - p)
};
inline DropArgs dropout_args(float p, uint64_t seed, const uint64_t *d_step) { return DropArgs{seed, d_step, dropout_thresh(p), dropout_scale(p)}; }
// p negative, NaN or >= 1, or a step word that is not 8-byte aligned
inline bool dropout_bad(float p, const void *d_step) { return !(p >= 0.0f) || !(p < 1.0f) || (reinterpret_cast<uintptr_t>(d_step) & 7) != 0; }

}  // namespace sx
