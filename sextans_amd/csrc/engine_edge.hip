// engine_edge.hip -- SpMM with a feature vector per stored entry over the CSR pattern on an engine handle (include/sextans_amd.h):
//   sextans_spmm_edge_device_rm            C[r, :] = sum over row r's entries of B[c, :] (op) E[e, :]   (mul / add / relu(add) / copy)
//   sextans_spmm_edge_backward_device_rm   dB and dE from the upstream gradient: a column pass over A^T, a row pass over A
// Kernels: spmm_edge_kernels.h on the row walking of pattern_pass.h; the entry points' frame: pattern_launch.h; the checks and the passes
// of both entry points: edge_launch.h, here for fp32 edge tensors (bf16: engine_edge_bf16.hip).  Only the pattern is read: neither the
// engine's values nor any of its packed forms is read or touched.
#include "edge_launch.h"

using namespace sxe;

extern "C" {

int sextans_spmm_edge_device_rm(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const float *d_E, int64_t lde,
                                float *d_C, int64_t ldc, void *stream) {
    return spmm_edge_forward<float>(h, op, N, d_B, ldb, d_E, lde, d_C, ldc, stream, "spmm_edge");
}

int sextans_spmm_edge_backward_device_rm(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const float *d_E, int64_t lde,
                                         const float *d_G, int64_t ldg, float *d_dB, int64_t lddb, float *d_dE, int64_t ldde, void *stream) {
    return spmm_edge_backward<float>(h, op, N, d_B, ldb, d_E, lde, d_G, ldg, d_dB, lddb, d_dE, ldde, stream, "spmm_edge_backward");
}

}  // extern "C"
