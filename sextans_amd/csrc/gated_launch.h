// gated_launch.h -- what the objects of the gated aggregation share: the launcher and the bodies of the two entry points, for one element
// type ET of the (nnz, N) tensors E, z, Gz and dE (spmm_gated_kernels.h).  engine_gated.hip instantiates ET = float
// (sextans_spmm_gated_device_rm, sextans_spmm_gated_backward_device_rm, and the workspace size, which serves both element types),
// engine_gated_bf16.hip and engine_gated_bf16_backward.hip ET = uint16_t (the _bf16 entry points): the kernels of one element type and
// direction are compiled in one object each, the checks, their order and the passes are one text.
#pragma once
#include "pattern_launch.h"
#include "spmm_gated_kernels.h"

namespace sxe {

// gn = G / (den + eps) into the M x N workspace (leading dimension N), fp32 for either element type: the kernel and this launcher are
// defined once, in engine_gated.hip
void gated_normalize(int64_t M, int N, const float *d_G, int64_t ldg, const float *d_den, int64_t ldden, float eps, float *d_gn, hipStream_t s);

namespace {

// e: the engine whose CSR arrays and softmax tables the pass walks (the column pass: the companion).  N is cut into tiles of the smallest
// of 8 / 16 / 32 / 64 floats that holds min(N, kMaxTile); the last tile may be partial; the tiles sit in the grid in every pass (an (entry,
// tile) of z and dE belongs to one slot).  The tile is capped at 64 floats as engine_multi.hip's is and for its reason: the forward keeps
// 2 W floats of state and the own xdst pieces next to up to three loaded tiles per entry in flight, the column pass up to five.
// Entries in flight per slot (U): 4 in the forward (three loads per entry), 2 in the backward passes (four and five); UNTUNED -- chosen from
// the resource listing (profiles/spmm_gated_kernel_resources.txt): no scratch, no spills at any width.
// The slot geometry does NOT depend on ET: the order of every sum, and with it every fp32 bit, is the same for both element types
// (bf16: profiles/gated_bf16_kernel_resources.txt).
constexpr int kMaxTile = 64;

template <int PASS, class ET>
void launch_pass(const sextans_engine *e, const sx::GatedArgsT<ET> &a, const int *perm, hipStream_t s) {
    for_width(a.N < kMaxTile ? a.N : kMaxTile, [&](auto w) {
        using W = decltype(w);
        constexpr int U = PASS == sx::kAttnForward ? 4 : 2;
        if constexpr (4 * W::T * W::P <= kMaxTile) launch_pattern<sx::GatedPass<PASS, W::T, W::P, U, ET>>(e, tiled<W>(a), perm, false, s);
    });
}

inline bool bad_mode(int mode) { return mode != SEXTANS_GATE_SUM && mode != SEXTANS_GATE_NORM; }
inline bool bad_eps(int mode, float eps) { return mode == SEXTANS_GATE_NORM && (!(eps > 0.0f) || std::isinf(eps)); }
// the operand struct (sextans_gated_in or sextans_gated_in_bf16): xdst, xsrc and V with their leading dimensions always, E's when it is
// given.  Leading dimensions are counted in elements of their tensor and are multiples of 4 for either element type (a bf16 piece is 8
// bytes).
template <class In>
bool bad_in(const In *in, int N) {
    return bad_ld(in->ld_xdst, N) || bad_ld(in->ld_xsrc, N) || bad_ld(in->ld_v, N) || bad_ld_of(in->d_e, in->ld_e, N) ||
           misaligned(in->d_xdst, in->d_xsrc, in->d_v, in->d_e);
}

// The forward entry point; name: what sextans_last_kernel reads afterwards.
template <class ET, class In>
int gated_forward(sextans_handle_t h, int mode, float eps, int N, const In *in, float *d_C, int64_t ldc, float *d_den, int64_t ldden, ET *d_z,
                  int64_t ldz, void *stream, const char *name) {
    if (!h || !in || bad_mode(mode) || bad_eps(mode, eps) || bad_n(N) || too_many_tiles(N, kMaxTile)) return SEXTANS_ERR_INVALID;   // nothing here needs a device
    if (bad_in(in, N) || bad_ld(ldc, N) || bad_ld_of(d_den, ldden, N) || bad_ld_of(d_z, ldz, N)) return SEXTANS_ERR_INVALID;
    if (misaligned(d_C, d_den, d_z)) return SEXTANS_ERR_INVALID;
    PatternCall call{h};
    if (int rc = call.open(!in->d_xdst || !in->d_xsrc || !in->d_v || !d_C, stream)) return rc;
    if (call.degenerate()) {   // every row is empty (z has no element)
        attention_fill(d_C, h->M, N, ldc, 0.0f, call.s);
        attention_fill(d_den, h->M, N, ldden, 0.0f, call.s);
        return call.done();
    }
    if (int rc = call.tables(false)) return rc;
    sx::GatedArgsT<ET> a{};
    a.xdst = in->d_xdst; a.xsrc = in->d_xsrc; a.V = in->d_v; a.E = in->d_e;
    a.ld_xdst = in->ld_xdst; a.ld_xsrc = in->ld_xsrc; a.ld_v = in->ld_v; a.ld_e = in->ld_e;
    a.out = d_C; a.den = d_den; a.z = d_z; a.ldc = ldc; a.ldden = ldden; a.ldz = ldz;
    a.norm = mode == SEXTANS_GATE_NORM; a.eps = eps; a.N = N;
    call.rows([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnForward>(e, a, perm, call.s); });
    return call.close(name);
}

template <class ET, class In, class Grad>
int gated_backward(sextans_handle_t h, int mode, float eps, int N, const In *in, const float *d_C, int64_t ldc, const float *d_den, int64_t ldden,
                   const float *d_G, int64_t ldg, const ET *d_Gz, int64_t ldgz, const Grad *out, float *d_work, void *stream, const char *name) {
    if (!h || !in || !out || bad_mode(mode) || bad_eps(mode, eps) || bad_n(N) || too_many_tiles(N, kMaxTile)) return SEXTANS_ERR_INVALID;
    const bool norm = mode == SEXTANS_GATE_NORM;
    if (!norm) d_C = d_den = nullptr;   // SUM ignores them
    if (bad_in(in, N) || bad_ld_of(d_C, ldc, N) || bad_ld_of(d_den, ldden, N) || bad_ld(ldg, N) || bad_ld_of(d_Gz, ldgz, N)) return SEXTANS_ERR_INVALID;
    if (bad_ld_of(out->d_dxdst, out->ld_dxdst, N) || bad_ld_of(out->d_dxsrc, out->ld_dxsrc, N) || bad_ld_of(out->d_dv, out->ld_dv, N) ||
        bad_ld_of(out->d_de, out->ld_de, N))
        return SEXTANS_ERR_INVALID;
    if (misaligned(d_C, d_den, d_G, d_Gz, out->d_dxdst, out->d_dxsrc, out->d_dv, out->d_de, d_work)) return SEXTANS_ERR_INVALID;
    if (!out->d_dxdst && !out->d_dxsrc && !out->d_dv && !out->d_de) return SEXTANS_ERR_INVALID;   // nothing to compute
    PatternCall call{h};
    if (int rc = call.open(!in->d_xdst || !in->d_xsrc || !in->d_v || !d_G || (norm && (!d_C || !d_den || !d_work)), stream)) return rc;
    if (call.degenerate()) {   // (dE has no element)
        attention_fill(out->d_dxdst, h->M, N, out->ld_dxdst, 0.0f, call.s);
        attention_fill(out->d_dxsrc, h->K, N, out->ld_dxsrc, 0.0f, call.s);
        attention_fill(out->d_dv, h->K, N, out->ld_dv, 0.0f, call.s);
        return call.done();
    }
    const bool rows = out->d_dxdst || out->d_de, cols = out->d_dxsrc || out->d_dv;
    if (int rc = call.tables(cols)) return rc;
    sx::GatedArgsT<ET> a{};
    a.xdst = in->d_xdst; a.xsrc = in->d_xsrc; a.V = in->d_v; a.E = in->d_e;
    a.ld_xdst = in->ld_xdst; a.ld_xsrc = in->ld_xsrc; a.ld_v = in->ld_v; a.ld_e = in->ld_e;
    a.C = d_C; a.ldc = ldc; a.Gz = d_Gz; a.ldgz = ldgz;
    a.gn = d_G; a.ldgn = ldg;
    a.dxdst = out->d_dxdst; a.dxsrc = out->d_dxsrc; a.dV = out->d_dv; a.dE = out->d_de;
    a.ld_dxdst = out->ld_dxdst; a.ld_dxsrc = out->ld_dxsrc; a.ld_dv = out->ld_dv; a.ld_de = out->ld_de;
    a.norm = norm; a.eps = eps; a.N = N;
    if (norm) {   // gn once, for both passes
        gated_normalize(h->M, N, d_G, ldg, d_den, ldden, eps, d_work, call.s);
        a.gn = d_work; a.ldgn = N;
    }
    if (cols) call.cols([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnBackwardCols>(e, a, perm, call.s); });
    if (rows) call.rows([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnBackwardRows>(e, a, perm, call.s); });
    return call.close(name);
}

}  // namespace
}  // namespace sxe
