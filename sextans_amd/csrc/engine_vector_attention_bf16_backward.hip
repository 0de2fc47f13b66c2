// engine_vector_attention_bf16_backward.hip -- the backward of the channel-wise attention with the (nnz, N) tensors in bf16
// (include/sextans_amd.h):
//   sextans_vector_attention_backward_device_rm_bf16   S, D, dS and dD bf16; V, C, lse, G and dV fp32
// (the forward: engine_vector_attention_bf16.hip).  The column pass and the row pass of engine_vector_attention.hip in the same order
// (vector_attention_launch.h, vector_attention_kernels.h with ET = uint16_t): S and D are widened exactly, every operation and sum is
// fp32, dS and dD are the fp32 results rounded once to nearest even -- dV is the fp32 entry point's bits on the widened S and D, dS and
// dD its dS and dD rounded.  2 messages x 4 widths x 2 kernels for dV, 3 x 4 x 2 for dS and dD: 40.
#include "vector_attention_launch.h"

using namespace sxe;

extern "C" {

int sextans_vector_attention_backward_device_rm_bf16(sextans_handle_t h, int msg, int N, const uint16_t *d_S, int64_t lds, const float *d_V,
                                                     int64_t ldv, const uint16_t *d_D, int64_t ldd, const float *d_C, int64_t ldc,
                                                     const float *d_lse, int64_t ldlse, const float *d_G, int64_t ldg, uint16_t *d_dS,
                                                     int64_t ldds, float *d_dV, int64_t lddv, uint16_t *d_dD, int64_t lddd, void *stream) {
    return vector_attention_backward<uint16_t>(h, msg, N, d_S, lds, d_V, ldv, d_D, ldd, d_C, ldc, d_lse, ldlse, d_G, ldg, d_dS, ldds, d_dV,
                                               lddv, d_dD, lddd, stream, "vector_attention_backward_bf16");
}

}  // extern "C"
