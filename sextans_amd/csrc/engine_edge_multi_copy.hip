// engine_edge_multi_copy.hip -- the kernels of the edge-feature multi-aggregation (engine_edge_multi.hip) for the message E[e] (no column pass):
// every pass, group and width of this op.  One source per op: see edge_multi_launch.h.
#include "edge_multi_launch.h"

namespace sxe {

void launch_edge_multi_copy(int pass, int groups, const sextans_engine *e, const sx::EdgeMultiArgs &a, const int *perm, hipStream_t s) {
    edge_multi_op<sx::kEdgeCopy>(pass, groups, e, a, perm, s);
}

}  // namespace sxe
