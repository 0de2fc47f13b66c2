// engine_edge_op_bf16.hip -- the edge-output ops of engine_edge_op.hip with the (nnz, N) tensors in bf16 (include/sextans_amd.h), forward:
//   sextans_edge_op_device_rm_bf16            E (optional) and Z bf16, x_dst and x_src fp32
// (the backward, sextans_edge_op_backward_device_rm_bf16: engine_edge_op_bf16_backward.hip -- the two passes' kernels are compiled in an
// object each, so that neither takes longer to build than the largest object there was).
// The same pass, slot geometry and operations (edge_op_launch.h, edge_op_kernels.h with ET = uint16_t): a bf16 value read is widened
// exactly, every operation is fp32, a bf16 value written is the fp32 result rounded once to nearest even -- so Z is the fp32 entry
// point's Z on the widened E, rounded.  5 ops x with / without E x 5 widths x 2 kernels: 100.
#include "edge_op_launch.h"

using namespace sxe;

extern "C" {

int sextans_edge_op_device_rm_bf16(sextans_handle_t h, int op, int N, const float *d_xdst, int64_t ldxdst, const float *d_xsrc, int64_t ldxsrc,
                                   const uint16_t *d_E, int64_t lde, uint16_t *d_Z, int64_t ldz, void *stream) {
    return edge_op_forward<uint16_t>(h, op, N, d_xdst, ldxdst, d_xsrc, ldxsrc, d_E, lde, d_Z, ldz, stream, "edge_op_bf16");
}

}  // extern "C"
