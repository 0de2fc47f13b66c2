// engine_vector_attention.hip -- channel-wise attention from per-channel scores over the CSR pattern on an engine handle
// (include/sextans_amd.h):
//   sextans_vector_attention_device_rm            C[r, n] = sum_e softmax_e(S[e, n])[n] m_e over row r's messages m_e = V[c, n] |
//                                                 V[c, n] + D[e, n] | D[e, n] (msg: SEXTANS_VATT_*), and lse
//   sextans_vector_attention_backward_device_rm   dS, dD and dV from C, lse and the upstream gradient: a row pass over A that stores dS and
//                                                 dD, a column pass over A^T for dV
// Kernels: vector_attention_kernels.h on the row walking of pattern_pass.h; the entry points' frame: pattern_launch.h; the checks and the
// passes of both entry points: vector_attention_launch.h, here for fp32 edge tensors (bf16: engine_vector_attention_bf16.hip and
// engine_vector_attention_bf16_backward.hip).  Only the pattern is read: neither the engine's values nor any of its packed forms is read
// or touched.
// All 3 passes x 3 messages x 4 widths x 2 kernels (less EDGE's column pass: 64) are instantiated here.
#include "vector_attention_launch.h"

using namespace sxe;

extern "C" {

int sextans_vector_attention_device_rm(sextans_handle_t h, int msg, int N, const float *d_S, int64_t lds, const float *d_V, int64_t ldv,
                                       const float *d_D, int64_t ldd, float *d_C, int64_t ldc, float *d_lse, int64_t ldlse, void *stream) {
    return vector_attention_forward<float>(h, msg, N, d_S, lds, d_V, ldv, d_D, ldd, d_C, ldc, d_lse, ldlse, stream, "vector_attention");
}

int sextans_vector_attention_backward_device_rm(sextans_handle_t h, int msg, int N, const float *d_S, int64_t lds, const float *d_V, int64_t ldv,
                                                const float *d_D, int64_t ldd, const float *d_C, int64_t ldc, const float *d_lse, int64_t ldlse,
                                                const float *d_G, int64_t ldg, float *d_dS, int64_t ldds, float *d_dV, int64_t lddv,
                                                float *d_dD, int64_t lddd, void *stream) {
    return vector_attention_backward<float>(h, msg, N, d_S, lds, d_V, ldv, d_D, ldd, d_C, ldc, d_lse, ldlse, d_G, ldg, d_dS, ldds, d_dV, lddv,
                                            d_dD, lddd, stream, "vector_attention_backward");
}

}  // extern "C"
