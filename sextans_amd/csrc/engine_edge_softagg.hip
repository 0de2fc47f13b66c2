// engine_edge_softagg.hip -- softmax aggregation of edge-feature messages over the CSR pattern on an engine handle (include/sextans_amd.h):
//   sextans_spmm_edge_softagg_device_rm            C[r, n] = sum_e softmax_e(t[n] m_e)[n] m_e over row r's messages m_e = B[c, n] (op) E[e, n]
//                                                  (mul / add / relu(add) / copy), and lse
//   sextans_spmm_edge_softagg_workspace_floats     the floats of workspace dt needs (dt_rows, then the chunk sums), for either element type
//   sextans_spmm_edge_softagg_backward_device_rm   dB, dE and dt from C, lse and the upstream gradient: a column pass over A^T, a row pass
//                                                  over A, the two-level dt sum
// Kernels: spmm_edge_softagg_kernels.h on the row walking of pattern_pass.h; the entry points' frame: pattern_launch.h; the checks and the
// passes of both entry points: edge_softagg_launch.h, here for fp32 edge tensors (bf16: engine_edge_softagg_bf16.hip and
// engine_edge_softagg_bf16_backward.hip).  Only the pattern is read: neither the engine's values nor any of its packed forms is read or
// touched.
// All 3 passes x 4 ops x 4 widths x 2 kernels (less COPY's column pass: 88) are instantiated here: the object compiles in less time than
// engine_multi.hip's, so it is not split by op as the edge multi-aggregation's is.
#include "edge_softagg_launch.h"

using namespace sxe;

extern "C" {

int sextans_spmm_edge_softagg_device_rm(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const float *d_E, int64_t lde,
                                        const float *d_t, float *d_C, int64_t ldc, float *d_lse, int64_t ldlse, void *stream) {
    return edge_softagg_forward<float>(h, op, N, d_B, ldb, d_E, lde, d_t, d_C, ldc, d_lse, ldlse, stream, "spmm_edge_softagg");
}

int64_t sextans_spmm_edge_softagg_workspace_floats(sextans_handle_t h, int N) {
    if (!h || bad_n(N) || too_many_tiles(N, kMaxTile)) return -(int64_t)SEXTANS_ERR_INVALID;
    if (!h->d_rp) return -(int64_t)SEXTANS_ERR_STATE;
    return (int64_t)h->M * N + chunks_of(h->M) * N;
}

int sextans_spmm_edge_softagg_backward_device_rm(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const float *d_E, int64_t lde,
                                                 const float *d_t, const float *d_C, int64_t ldc, const float *d_lse, int64_t ldlse,
                                                 const float *d_G, int64_t ldg, float *d_dB, int64_t lddb, float *d_dE, int64_t ldde, float *d_dt,
                                                 float *d_work, void *stream) {
    return edge_softagg_backward<float>(h, op, N, d_B, ldb, d_E, lde, d_t, d_C, ldc, d_lse, ldlse, d_G, ldg, d_dB, lddb, d_dE, ldde, d_dt,
                                        d_work, stream, "spmm_edge_softagg_backward");
}

}  // extern "C"
