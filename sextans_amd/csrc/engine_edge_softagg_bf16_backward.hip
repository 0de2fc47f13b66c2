// engine_edge_softagg_bf16_backward.hip -- the backward of the edge-feature softmax aggregation with the (nnz, N) tensors in bf16
// (include/sextans_amd.h):
//   sextans_spmm_edge_softagg_backward_device_rm_bf16   E and dE bf16; B, t, C, lse, G, dB, dt and the workspace fp32
// (the forward: engine_edge_softagg_bf16.hip; the workspace size: sextans_spmm_edge_softagg_workspace_floats, one for both element types).
// The column pass, the row pass and the dt sum of engine_edge_softagg.hip in the same order (edge_softagg_launch.h,
// spmm_edge_softagg_kernels.h with ET = uint16_t): E is widened exactly, every operation and sum is fp32, dE is the fp32 result rounded
// once to nearest even -- dB and dt are the fp32 entry point's bits on the widened E, dE its dE rounded.
// 3 ops x 4 widths x 2 kernels for dB, 4 x 4 x 2 for dE and dt: 56.
#include "edge_softagg_launch.h"

using namespace sxe;

extern "C" {

int sextans_spmm_edge_softagg_backward_device_rm_bf16(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const uint16_t *d_E,
                                                      int64_t lde, const float *d_t, const float *d_C, int64_t ldc, const float *d_lse,
                                                      int64_t ldlse, const float *d_G, int64_t ldg, float *d_dB, int64_t lddb, uint16_t *d_dE,
                                                      int64_t ldde, float *d_dt, float *d_work, void *stream) {
    return edge_softagg_backward<uint16_t>(h, op, N, d_B, ldb, d_E, lde, d_t, d_C, ldc, d_lse, ldlse, d_G, ldg, d_dB, lddb, d_dE, ldde, d_dt,
                                           d_work, stream, "spmm_edge_softagg_backward_bf16");
}

}  // extern "C"
