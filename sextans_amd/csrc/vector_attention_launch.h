// vector_attention_launch.h -- what the objects of the channel-wise attention share: the launchers and the bodies of the two entry
// points, for one element type ET of the (nnz, N) tensors S, D, dS and dD (vector_attention_kernels.h).  engine_vector_attention.hip
// instantiates ET = float (sextans_vector_attention_device_rm, sextans_vector_attention_backward_device_rm),
// engine_vector_attention_bf16.hip and engine_vector_attention_bf16_backward.hip ET = uint16_t (the _bf16 entry points): the kernels of
// one element type and direction are compiled in one object each, the checks, their order and the passes are one text.
// The row pass runs when dS or dD is asked for, the column pass (and the transpose) only for dV.  The row pass's two stores are
// PREDICATED on their pointers, not compile-time switches, as edge_softagg_launch.h's dE store is and for its reason.
#pragma once
#include "pattern_launch.h"
#include "vector_attention_kernels.h"

namespace sxe {
namespace {

// e: the engine whose CSR arrays and softmax tables the pass walks (the column pass: the companion).  N is cut into tiles of the smallest
// of 8 / 16 / 32 / 64 floats that holds min(N, kMaxTile); the last tile may be partial; the tiles sit in the grid in every pass.  The
// tile is capped at 64 floats as edge_softagg_launch.h's is: these passes carry an S row per entry in flight on top of its streams.
// Entries in flight per slot (U), all UNTUNED -- no other value has been timed: 4 in the forward (it MUST equal engine_softagg.hip's
// and edge_softagg_launch.h's 4: fed S = t[n] m_e the forward then returns those families' bits, which
// tests/test_vector_attention_gpu.py pins), 4 in the row pass (an entry costs its S row, a gathered V row and its D row), 4 in the
// column pass (its S row through perm and two gathered rows, lse and G -- one row fewer than the parent's column pass and no message to
// recompute).  No kernel uses scratch or spills at these values (profiles/vector_attention_kernel_resources.txt).
// The slot geometry does NOT depend on ET: the order of every sum, and with it every fp32 bit, is the same for both element types.
constexpr int kMaxTile = 64;

template <int PASS, int MSG, class ET>
void launch_pass(const sextans_engine *e, const sx::VectorAttnArgsT<ET> &a, const int *perm, hipStream_t s) {
    for_width(a.N < kMaxTile ? a.N : kMaxTile, [&](auto w) {
        using W = decltype(w);
        constexpr int U = 4;
        if constexpr (4 * W::T * W::P <= kMaxTile) launch_pattern<sx::VectorAttnPass<PASS, MSG, W::T, W::P, U, ET>>(e, tiled<W>(a), perm, false, s);
    });
}

template <int PASS, class ET>
void launch_msg(int msg, const sextans_engine *e, const sx::VectorAttnArgsT<ET> &a, const int *perm, hipStream_t s) {
    if (msg == SEXTANS_VATT_NODE) launch_pass<PASS, sx::kVattNode>(e, a, perm, s);
    else if (msg == SEXTANS_VATT_ADD) launch_pass<PASS, sx::kVattAdd>(e, a, perm, s);
    else if constexpr (PASS != sx::kAttnBackwardCols) launch_pass<PASS, sx::kVattEdge>(e, a, perm, s);   // (EDGE has no dV)
}

inline bool bad_msg(int msg) { return msg < SEXTANS_VATT_NODE || msg > SEXTANS_VATT_EDGE; }
inline bool reads_v(int msg) { return msg != SEXTANS_VATT_EDGE; }
inline bool reads_d(int msg) { return msg != SEXTANS_VATT_NODE; }

// The forward entry point; name: what sextans_last_kernel reads afterwards.  Leading dimensions are counted in elements of their tensor
// and are multiples of 4 for either element type (a bf16 piece is 8 bytes).
template <class ET>
int vector_attention_forward(sextans_handle_t h, int msg, int N, const ET *d_S, int64_t lds, const float *d_V, int64_t ldv, const ET *d_D,
                             int64_t ldd, float *d_C, int64_t ldc, float *d_lse, int64_t ldlse, void *stream, const char *name) {
    if (!h || bad_msg(msg) || bad_n(N) || too_many_tiles(N, kMaxTile)) return SEXTANS_ERR_INVALID;   // nothing here needs a device
    if (!reads_v(msg)) d_V = nullptr;   // an operand the mode does not read is ignored, with its leading dimension
    if (!reads_d(msg)) d_D = nullptr;
    if (bad_ld(lds, N) || (reads_v(msg) && bad_ld(ldv, N)) || (reads_d(msg) && bad_ld(ldd, N)) || bad_ld(ldc, N) || bad_ld_of(d_lse, ldlse, N))
        return SEXTANS_ERR_INVALID;
    if (misaligned(d_S, d_V, d_D, d_C, d_lse)) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    if (int rc = call.open(!d_S || (reads_v(msg) && !d_V) || (reads_d(msg) && !d_D) || !d_C, stream)) return rc;
    if (call.degenerate()) {   // every row is empty
        attention_fill(d_C, h->M, N, ldc, 0.0f, call.s);
        attention_fill(d_lse, h->M, N, ldlse, -INFINITY, call.s);
        return call.done();
    }
    if (int rc = call.tables(false)) return rc;
    sx::VectorAttnArgsT<ET> a{};
    a.S = d_S; a.V = d_V; a.D = d_D; a.out = d_C; a.out_lse = d_lse;
    a.lds = lds; a.ldv = ldv; a.ldd = ldd; a.ldc = ldc; a.ldlse = ldlse; a.N = N;
    call.rows([&](const sextans_engine *e, const int *perm) { launch_msg<sx::kAttnForward>(msg, e, a, perm, call.s); });
    return call.close(name);
}

template <class ET>
int vector_attention_backward(sextans_handle_t h, int msg, int N, const ET *d_S, int64_t lds, const float *d_V, int64_t ldv, const ET *d_D,
                              int64_t ldd, const float *d_C, int64_t ldc, const float *d_lse, int64_t ldlse, const float *d_G, int64_t ldg,
                              ET *d_dS, int64_t ldds, float *d_dV, int64_t lddv, ET *d_dD, int64_t lddd, void *stream, const char *name) {
    if (!h || bad_msg(msg) || bad_n(N) || too_many_tiles(N, kMaxTile)) return SEXTANS_ERR_INVALID;
    if (!reads_v(msg)) d_V = nullptr;
    if (!reads_d(msg)) d_D = nullptr;
    if (bad_ld(lds, N) || (reads_v(msg) && bad_ld(ldv, N)) || (reads_d(msg) && bad_ld(ldd, N)) || bad_ld(ldc, N) || bad_ld(ldlse, N) ||
        bad_ld(ldg, N) || bad_ld_of(d_dS, ldds, N) || bad_ld_of(d_dV, lddv, N) || bad_ld_of(d_dD, lddd, N))
        return SEXTANS_ERR_INVALID;
    if (misaligned(d_S, d_V, d_D, d_C, d_lse, d_G, d_dS, d_dV, d_dD)) return SEXTANS_ERR_INVALID;
    if (!d_dS && !d_dV && !d_dD) return SEXTANS_ERR_INVALID;   // nothing to compute
    if (d_dV && !reads_v(msg)) return SEXTANS_ERR_INVALID;     // a gradient of an operand the mode does not read
    if (d_dD && !reads_d(msg)) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    if (int rc = call.open(!d_S || (reads_v(msg) && !d_V) || (reads_d(msg) && !d_D) || !d_C || !d_lse || !d_G, stream)) return rc;
    if (call.degenerate()) {   // (dS and dD have no element)
        attention_fill(d_dV, h->K, N, lddv, 0.0f, call.s);
        return call.done();
    }
    if (int rc = call.tables(d_dV != nullptr)) return rc;
    sx::VectorAttnArgsT<ET> a{};
    a.S = d_S; a.V = d_V; a.D = d_D; a.C = d_C; a.lse = d_lse; a.G = d_G;
    a.dS = d_dS; a.dV = d_dV; a.dD = d_dD;
    a.lds = lds; a.ldv = ldv; a.ldd = ldd; a.ldc = ldc; a.ldlse = ldlse; a.ldg = ldg; a.ldds = ldds; a.lddv = lddv; a.lddd = lddd; a.N = N;
    if (d_dV) call.cols([&](const sextans_engine *e, const int *perm) { launch_msg<sx::kAttnBackwardCols>(msg, e, a, perm, call.s); });
    if (d_dS || d_dD) call.rows([&](const sextans_engine *e, const int *perm) { launch_msg<sx::kAttnBackwardRows>(msg, e, a, perm, call.s); });
    return call.close(name);
}

}  // namespace
}  // namespace sxe
