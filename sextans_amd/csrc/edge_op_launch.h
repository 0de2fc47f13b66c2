// edge_op_launch.h -- what the two objects of the edge-output ops share: the launchers and the bodies of the two entry points, for one
// element type ET of the (nnz, N) tensors E, Z and Gz (edge_op_kernels.h).  engine_edge_op.hip instantiates ET = float
// (sextans_edge_op_device_rm, sextans_edge_op_backward_device_rm), engine_edge_op_bf16.hip ET = uint16_t (the _bf16 entry points): the
// kernels of one element type are compiled in one object each, the checks, their order and the passes are one text.
#pragma once
#include "edge_op_kernels.h"
#include "pattern_launch.h"

namespace sxe {
namespace {

// e: the engine whose CSR arrays and softmax tables the pass walks (dx_src: the companion).  N is cut into tiles of the smallest of
// 8 / 16 / 32 / 64 / 128 floats that holds min(N, 128), engine_edge.hip's cut; the last tile may be partial; the tiles sit in the grid in
// every pass.  Entries in flight per slot (U): engine_edge.hip's 4 (2 at width 128) in both passes -- an entry costs up to two loads of
// a tile's pieces (x_src and E; Gz and the other endpoint) on top of the own row's pieces or the sums.  UNTUNED: no other value has been
// timed.  No kernel uses scratch or spills at these values (profiles/edge_op_kernel_resources.txt; bf16:
// profiles/edge_bf16_kernel_resources.txt).
template <int OP, bool HAS_E, class ET>
void launch_forward(const sextans_engine *e, const sx::EdgeOpArgsT<ET> &a, hipStream_t s) {
    for_width(a.N, [&](auto w) {
        using W = decltype(w);
        launch_pattern<sx::EdgeOpPass<OP, HAS_E, W::T, W::P, W::k128 ? 2 : 4, ET>>(e, tiled<W>(a), nullptr, false, s);
    });
}

template <int OP, class ET>
void launch_forward_e(const sextans_engine *e, const sx::EdgeOpArgsT<ET> &a, hipStream_t s) {
    if (a.E) launch_forward<OP, true>(e, a, s);
    else launch_forward<OP, false>(e, a, s);
}

template <class ET>
void launch_forward_op(int op, const sextans_engine *e, const sx::EdgeOpArgsT<ET> &a, hipStream_t s) {
    if (op == SEXTANS_EDGEOP_ADD) launch_forward_e<sx::kEdgeOpAdd>(e, a, s);
    else if (op == SEXTANS_EDGEOP_SUB) launch_forward_e<sx::kEdgeOpSub>(e, a, s);
    else if (op == SEXTANS_EDGEOP_MUL) launch_forward_e<sx::kEdgeOpMul>(e, a, s);
    else if (op == SEXTANS_EDGEOP_DST) launch_forward_e<sx::kEdgeOpDst>(e, a, s);
    else launch_forward_e<sx::kEdgeOpSrc>(e, a, s);
}

template <int TERM, bool PERM, class ET>
void launch_sum(const sextans_engine *e, const sx::EdgeOpArgsT<ET> &a, const int *perm, hipStream_t s) {
    for_width(a.N, [&](auto w) {
        using W = decltype(w);
        launch_pattern<sx::EndpointSumPass<TERM, PERM, W::T, W::P, W::k128 ? 2 : 4, ET>>(e, tiled<W>(a), perm, false, s);
    });
}

// perm: NULL on A's own arrays (dx_dst), the transpose's permutation on A^T's (dx_src)
template <class ET>
void launch_sum_term(int term, const sextans_engine *e, const sx::EdgeOpArgsT<ET> &a, const int *perm, hipStream_t s) {
    if (perm) {
        if (term == sx::kEndSumMul) launch_sum<sx::kEndSumMul, true>(e, a, perm, s);
        else if (term == sx::kEndSumNeg) launch_sum<sx::kEndSumNeg, true>(e, a, perm, s);
        else launch_sum<sx::kEndSumPlain, true>(e, a, perm, s);
    } else {
        if (term == sx::kEndSumMul) launch_sum<sx::kEndSumMul, false>(e, a, perm, s);
        else if (term == sx::kEndSumNeg) launch_sum<sx::kEndSumNeg, false>(e, a, perm, s);
        else launch_sum<sx::kEndSumPlain, false>(e, a, perm, s);
    }
}

inline bool bad_op(int op) { return op < SEXTANS_EDGEOP_ADD || op > SEXTANS_EDGEOP_SRC; }
inline bool reads_dst(int op) { return op != SEXTANS_EDGEOP_SRC; }
inline bool reads_src(int op) { return op != SEXTANS_EDGEOP_DST; }

// The forward entry point; name: what sextans_last_kernel reads afterwards.  Leading dimensions are counted in elements of their tensor
// and are multiples of 4 for either element type (a bf16 piece is 8 bytes).
template <class ET>
int edge_op_forward(sextans_handle_t h, int op, int N, const float *d_xdst, int64_t ldxdst, const float *d_xsrc, int64_t ldxsrc, const ET *d_E,
                    int64_t lde, ET *d_Z, int64_t ldz, void *stream, const char *name) {
    if (!h || bad_op(op) || bad_n(N)) return SEXTANS_ERR_INVALID;   // nothing here needs a device
    if (!reads_dst(op)) d_xdst = nullptr;   // an operand the op does not read is ignored, with its leading dimension
    if (!reads_src(op)) d_xsrc = nullptr;
    if ((reads_dst(op) && bad_ld(ldxdst, N)) || (reads_src(op) && bad_ld(ldxsrc, N)) || bad_ld_of(d_E, lde, N) || bad_ld(ldz, N))
        return SEXTANS_ERR_INVALID;
    if (misaligned(d_xdst, d_xsrc, d_E, d_Z)) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    if (int rc = call.open((reads_dst(op) && !d_xdst) || (reads_src(op) && !d_xsrc) || !d_Z, stream)) return rc;
    if (call.degenerate()) return SEXTANS_OK;   // Z has no element
    if (int rc = call.tables(false)) return rc;
    sx::EdgeOpArgsT<ET> a{};
    a.xdst = d_xdst; a.xsrc = d_xsrc; a.E = d_E; a.Z = d_Z;
    a.ldxdst = ldxdst; a.ldxsrc = ldxsrc; a.lde = lde; a.ldz = ldz; a.N = N;
    call.rows([&](const sextans_engine *e, const int *) { launch_forward_op(op, e, a, call.s); });
    return call.close(name);
}

template <class ET>
int edge_op_backward(sextans_handle_t h, int op, int N, const float *d_xdst, int64_t ldxdst, const float *d_xsrc, int64_t ldxsrc, const ET *d_Gz,
                     int64_t ldgz, float *d_dxdst, int64_t lddxdst, float *d_dxsrc, int64_t lddxsrc, void *stream, const char *name) {
    if (!h || bad_op(op) || bad_n(N)) return SEXTANS_ERR_INVALID;
    // what the backward reads of the forward's operands: MUL alone, the OTHER endpoint of each gradient that is asked for
    const bool need_dst = op == SEXTANS_EDGEOP_MUL && d_dxsrc, need_src = op == SEXTANS_EDGEOP_MUL && d_dxdst;
    if (!need_dst) d_xdst = nullptr;
    if (!need_src) d_xsrc = nullptr;
    if ((need_dst && bad_ld(ldxdst, N)) || (need_src && bad_ld(ldxsrc, N)) || bad_ld(ldgz, N) || bad_ld_of(d_dxdst, lddxdst, N) ||
        bad_ld_of(d_dxsrc, lddxsrc, N))
        return SEXTANS_ERR_INVALID;
    if (misaligned(d_xdst, d_xsrc, d_Gz, d_dxdst, d_dxsrc)) return SEXTANS_ERR_INVALID;
    if (!d_dxdst && !d_dxsrc) return SEXTANS_ERR_INVALID;                    // nothing to compute
    if (d_dxdst && !reads_dst(op)) return SEXTANS_ERR_INVALID;               // a gradient of an operand the op does not read
    if (d_dxsrc && !reads_src(op)) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    if (int rc = call.open(!d_Gz || (need_dst && !d_xdst) || (need_src && !d_xsrc), stream)) return rc;
    if (call.degenerate()) {   // every row and column is empty
        attention_fill(d_dxdst, h->M, N, lddxdst, 0.0f, call.s);
        attention_fill(d_dxsrc, h->K, N, lddxsrc, 0.0f, call.s);
        return call.done();
    }
    if (int rc = call.tables(d_dxsrc != nullptr)) return rc;
    sx::EdgeOpArgsT<ET> a{};
    a.Gz = d_Gz; a.ldgz = ldgz; a.N = N;
    const int mul = op == SEXTANS_EDGEOP_MUL ? sx::kEndSumMul : sx::kEndSumPlain;
    if (d_dxsrc) {   // over A^T: own = c, the other endpoint r
        a.x = d_xdst; a.ldx = ldxdst; a.out = d_dxsrc; a.ldout = lddxsrc;
        const int term = op == SEXTANS_EDGEOP_SUB ? sx::kEndSumNeg : mul;
        call.cols([&](const sextans_engine *e, const int *perm) { launch_sum_term(term, e, a, perm, call.s); });
    }
    if (d_dxdst) {   // over A: own = r, the other endpoint c
        a.x = d_xsrc; a.ldx = ldxsrc; a.out = d_dxdst; a.ldout = lddxdst;
        call.rows([&](const sextans_engine *e, const int *perm) { launch_sum_term(mul, e, a, perm, call.s); });
    }
    return call.close(name);
}

}  // namespace
}  // namespace sxe
