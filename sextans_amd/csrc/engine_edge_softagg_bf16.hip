// engine_edge_softagg_bf16.hip -- the edge-feature softmax aggregation of engine_edge_softagg.hip with the (nnz, N) tensor in bf16
// (include/sextans_amd.h), forward:
//   sextans_spmm_edge_softagg_device_rm_bf16            E bf16; B, t, C and lse fp32
// (the backward, sextans_spmm_edge_softagg_backward_device_rm_bf16: engine_edge_softagg_bf16_backward.hip -- the directions' kernels are
// compiled in an object each, as engine_edge_bf16.hip's are).
// The same pass, slot geometry and order of every sum (edge_softagg_launch.h, spmm_edge_softagg_kernels.h with ET = uint16_t): E is
// widened exactly, every operation, the online-softmax state and its merges are fp32 -- C and lse are the fp32 entry point's bits on the
// widened E.  4 ops x 4 widths x 2 kernels: 32.
#include "edge_softagg_launch.h"

using namespace sxe;

extern "C" {

int sextans_spmm_edge_softagg_device_rm_bf16(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const uint16_t *d_E, int64_t lde,
                                             const float *d_t, float *d_C, int64_t ldc, float *d_lse, int64_t ldlse, void *stream) {
    return edge_softagg_forward<uint16_t>(h, op, N, d_B, ldb, d_E, lde, d_t, d_C, ldc, d_lse, ldlse, stream, "spmm_edge_softagg_bf16");
}

}  // extern "C"
