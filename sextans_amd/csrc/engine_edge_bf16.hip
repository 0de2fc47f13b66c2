// engine_edge_bf16.hip -- the edge-feature SpMM of engine_edge.hip with the (nnz, N) tensors in bf16 (include/sextans_amd.h), forward:
//   sextans_spmm_edge_device_rm_bf16            E bf16; B and C fp32
// (the backward, sextans_spmm_edge_backward_device_rm_bf16: engine_edge_bf16_backward.hip -- the passes' kernels are compiled in an object
// each, so that neither takes longer to build than the largest object there was).
// The same pass, slot geometry and order of every sum (edge_launch.h, spmm_edge_kernels.h with ET = uint16_t): E is widened exactly,
// every operation and sum is fp32 -- C is the fp32 entry point's bits on the widened E.  4 ops x 5 widths x 2 kernels: 40.
#include "edge_launch.h"

using namespace sxe;

extern "C" {

int sextans_spmm_edge_device_rm_bf16(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const uint16_t *d_E, int64_t lde,
                                     float *d_C, int64_t ldc, void *stream) {
    return spmm_edge_forward<uint16_t>(h, op, N, d_B, ldb, d_E, lde, d_C, ldc, stream, "spmm_edge_bf16");
}

}  // extern "C"
