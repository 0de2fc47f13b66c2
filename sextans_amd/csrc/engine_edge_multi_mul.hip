// engine_edge_multi_mul.hip -- the kernels of the edge-feature multi-aggregation (engine_edge_multi.hip) for the message B[c] * E[e]:
// every pass, group and width of this op.  One source per op: see edge_multi_launch.h.
#include "edge_multi_launch.h"

namespace sxe {

void launch_edge_multi_mul(int pass, int groups, const sextans_engine *e, const sx::EdgeMultiArgs &a, const int *perm, hipStream_t s) {
    edge_multi_op<sx::kEdgeMul>(pass, groups, e, a, perm, s);
}

}  // namespace sxe
