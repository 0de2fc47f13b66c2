// engine_vector_attention_bf16.hip -- the channel-wise attention of engine_vector_attention.hip with the (nnz, N) tensors in bf16
// (include/sextans_amd.h), forward:
//   sextans_vector_attention_device_rm_bf16            S and D bf16; V, C and lse fp32
// (the backward, sextans_vector_attention_backward_device_rm_bf16: engine_vector_attention_bf16_backward.hip -- the directions' kernels
// are compiled in an object each, as engine_edge_bf16.hip's are).
// The same pass, slot geometry and order of every sum (vector_attention_launch.h, vector_attention_kernels.h with ET = uint16_t): S and D
// are widened exactly -- a bf16 -inf score is still a mask --, every operation, the online-softmax state and its merges are fp32: C and
// lse are the fp32 entry point's bits on the widened S and D.  3 messages x 4 widths x 2 kernels: 24.
#include "vector_attention_launch.h"

using namespace sxe;

extern "C" {

int sextans_vector_attention_device_rm_bf16(sextans_handle_t h, int msg, int N, const uint16_t *d_S, int64_t lds, const float *d_V, int64_t ldv,
                                            const uint16_t *d_D, int64_t ldd, float *d_C, int64_t ldc, float *d_lse, int64_t ldlse,
                                            void *stream) {
    return vector_attention_forward<uint16_t>(h, msg, N, d_S, lds, d_V, ldv, d_D, ldd, d_C, ldc, d_lse, ldlse, stream, "vector_attention_bf16");
}

}  // extern "C"
