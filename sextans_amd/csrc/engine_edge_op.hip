// engine_edge_op.hip -- edge-output ops from both endpoints of every stored entry of the CSR pattern on an engine handle
// (include/sextans_amd.h):
//   sextans_edge_op_device_rm            Z[e, :] = x_dst[r, :] (op) x_src[c, :] (+ E[e, :]) for every stored entry e = (r, c)
//                                        (add / sub / mul / dst / src)
//   sextans_edge_op_backward_device_rm   dx_dst and dx_src from the upstream gradient Gz of Z: an endpoint sum over A's rows, the same
//                                        pass over A^T's rows through the transpose's permutation
// Kernels: edge_op_kernels.h on the row walking of pattern_pass.h; the entry points' frame: pattern_launch.h; the checks and the passes of
// both entry points: edge_op_launch.h, here for fp32 edge tensors (bf16: engine_edge_op_bf16.hip).  Only the pattern is read: neither
// the engine's values nor any of its packed forms is read or touched.  dE = Gz needs no kernel.
// 5 ops x with / without E x 5 widths x 2 kernels forward (100), 3 terms x 2 directions x 5 widths x 2 kernels backward (60).
#include "edge_op_launch.h"

using namespace sxe;

extern "C" {

int sextans_edge_op_device_rm(sextans_handle_t h, int op, int N, const float *d_xdst, int64_t ldxdst, const float *d_xsrc, int64_t ldxsrc,
                              const float *d_E, int64_t lde, float *d_Z, int64_t ldz, void *stream) {
    return edge_op_forward<float>(h, op, N, d_xdst, ldxdst, d_xsrc, ldxsrc, d_E, lde, d_Z, ldz, stream, "edge_op");
}

int sextans_edge_op_backward_device_rm(sextans_handle_t h, int op, int N, const float *d_xdst, int64_t ldxdst, const float *d_xsrc,
                                       int64_t ldxsrc, const float *d_Gz, int64_t ldgz, float *d_dxdst, int64_t lddxdst, float *d_dxsrc,
                                       int64_t lddxsrc, void *stream) {
    return edge_op_backward<float>(h, op, N, d_xdst, ldxdst, d_xsrc, ldxsrc, d_Gz, ldgz, d_dxdst, lddxdst, d_dxsrc, lddxsrc, stream,
                                   "edge_op_backward");
}

}  // extern "C"
