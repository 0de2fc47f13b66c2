// engine_edge_bf16_backward.hip -- the backward of the edge-feature SpMM with the (nnz, N) tensors in bf16 (include/sextans_amd.h):
//   sextans_spmm_edge_backward_device_rm_bf16   E and dE bf16; B, G and dB fp32
// (the forward: engine_edge_bf16.hip).  The column pass and the row pass of engine_edge.hip in the same order (edge_launch.h,
// spmm_edge_kernels.h with ET = uint16_t): E is widened exactly, every operation and sum is fp32, dE is the fp32 result rounded once to
// nearest even -- dB is the fp32 entry point's bits on the widened E, dE its dE rounded.
// 3 ops x 5 widths x 2 kernels for dB, 4 x 5 x 2 for dE: 70.
#include "edge_launch.h"

using namespace sxe;

extern "C" {

int sextans_spmm_edge_backward_device_rm_bf16(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const uint16_t *d_E,
                                              int64_t lde, const float *d_G, int64_t ldg, float *d_dB, int64_t lddb, uint16_t *d_dE,
                                              int64_t ldde, void *stream) {
    return spmm_edge_backward<uint16_t>(h, op, N, d_B, ldb, d_E, lde, d_G, ldg, d_dB, lddb, d_dE, ldde, stream, "spmm_edge_backward_bf16");
}

}  // extern "C"
