// engine_gated_bf16_backward.hip -- the backward of the gated aggregation with the (nnz, N) tensors in bf16 (include/sextans_amd.h):
//   sextans_spmm_gated_backward_device_rm_bf16   E, Gz and dE bf16; xdst, xsrc, V, C, den, G, dxdst, dxsrc, dV and the workspace fp32
// (the forward: engine_gated_bf16.hip; the workspace size: sextans_spmm_gated_workspace_floats, one for both element types; gn is written
// by engine_gated.hip's kernel).
// The column pass and the row pass of engine_gated.hip in the same order (gated_launch.h, spmm_gated_kernels.h with ET = uint16_t): E and
// Gz are widened exactly, the gate is recomputed from the unrounded z_e, every operation and sum is fp32 -- dxdst and dxsrc sum the
// unrounded dz_e --, and only the stored dE is rounded, once, to nearest even: dxdst, dxsrc and dV are the fp32 entry point's bits on the
// widened inputs, dE its dE rounded.  2 passes x 4 widths x 2 kernels: 16.
#include "gated_launch.h"

using namespace sxe;

extern "C" {

int sextans_spmm_gated_backward_device_rm_bf16(sextans_handle_t h, int mode, float eps, int N, const sextans_gated_in_bf16 *in, const float *d_C,
                                               int64_t ldc, const float *d_den, int64_t ldden, const float *d_G, int64_t ldg, const uint16_t *d_Gz,
                                               int64_t ldgz, const sextans_gated_grad_bf16 *out, float *d_work, void *stream) {
    return gated_backward<uint16_t>(h, mode, eps, N, in, d_C, ldc, d_den, ldden, d_G, ldg, d_Gz, ldgz, out, d_work, stream,
                                    "spmm_gated_backward_bf16");
}

}  // extern "C"
