// engine_edge_op_bf16_backward.hip -- the backward of the edge-output ops with the upstream gradient in bf16 (include/sextans_amd.h):
//   sextans_edge_op_backward_device_rm_bf16   Gz bf16, dx_dst and dx_src fp32
// (the forward: engine_edge_op_bf16.hip).  The endpoint sums of engine_edge_op.hip in the same order (edge_op_launch.h,
// edge_op_kernels.h with ET = uint16_t): Gz is widened exactly, every sum is fp32 -- dx_dst and dx_src are the fp32 entry point's bits on
// the widened Gz.  3 terms x 2 directions x 5 widths x 2 kernels: 60.
#include "edge_op_launch.h"

using namespace sxe;

extern "C" {

int sextans_edge_op_backward_device_rm_bf16(sextans_handle_t h, int op, int N, const float *d_xdst, int64_t ldxdst, const float *d_xsrc,
                                            int64_t ldxsrc, const uint16_t *d_Gz, int64_t ldgz, float *d_dxdst, int64_t lddxdst,
                                            float *d_dxsrc, int64_t lddxsrc, void *stream) {
    return edge_op_backward<uint16_t>(h, op, N, d_xdst, ldxdst, d_xsrc, ldxsrc, d_Gz, ldgz, d_dxdst, lddxdst, d_dxsrc, lddxsrc, stream,
                                      "edge_op_backward_bf16");
}

}  // extern "C"
