// engine_gated_bf16.hip -- the gated aggregation of engine_gated.hip with the (nnz, N) tensors in bf16 (include/sextans_amd.h), forward:
//   sextans_spmm_gated_device_rm_bf16            E and z bf16; xdst, xsrc, V, C and den fp32
// (the backward, sextans_spmm_gated_backward_device_rm_bf16: engine_gated_bf16_backward.hip -- the directions' kernels are compiled in an
// object each, as engine_edge_bf16.hip's are).
// The same pass, slot geometry and order of every sum (gated_launch.h, spmm_gated_kernels.h with ET = uint16_t): E is widened exactly,
// every operation and sum is fp32, the gate is taken from the unrounded z_e and only the stored copy of z is rounded, once, to nearest
// even -- C and den are the fp32 entry point's bits on the widened E, z its z rounded.  4 widths x 2 kernels: 8.
#include "gated_launch.h"

using namespace sxe;

extern "C" {

int sextans_spmm_gated_device_rm_bf16(sextans_handle_t h, int mode, float eps, int N, const sextans_gated_in_bf16 *in, float *d_C, int64_t ldc,
                                      float *d_den, int64_t ldden, uint16_t *d_z, int64_t ldz, void *stream) {
    return gated_forward<uint16_t>(h, mode, eps, N, in, d_C, ldc, d_den, ldden, d_z, ldz, stream, "spmm_gated_bf16");
}

}  // extern "C"
