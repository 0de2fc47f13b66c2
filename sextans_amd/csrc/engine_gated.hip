// engine_gated.hip -- gated aggregation over the CSR pattern on an engine handle (include/sextans_amd.h):
//   sextans_spmm_gated_device_rm            C[r, :] = sum over row r's entries of sigmoid(xdst[r] + xsrc[c] (+ E[e])) * V[c], as it is (SUM) or
//                                           divided by the sum of the gates + eps (NORM); optionally the gates' sum and the pre-activations z
//   sextans_spmm_gated_workspace_floats     the floats of workspace the backward needs (NORM: gn = G / (den + eps), M x N; SUM: none)
//   sextans_spmm_gated_backward_device_rm   dxdst and dE (a row pass over A), dxsrc and dV (a column pass over A^T), each only when asked for
// Kernels: spmm_gated_kernels.h on the row walking of pattern_pass.h; the entry points' frame: pattern_launch.h.  Only the pattern is
// read: neither the engine's values nor any of its packed forms is read or touched.
#include "pattern_launch.h"
#include "spmm_gated_kernels.h"

namespace sxe {
namespace {

// e: the engine whose CSR arrays and softmax tables the pass walks (the column pass: the companion).  N is cut into tiles of the smallest
// of 8 / 16 / 32 / 64 floats that holds min(N, kMaxTile); the last tile may be partial; the tiles sit in the grid in every pass (an (entry,
// tile) of z and dE belongs to one slot).  The tile is capped at 64 floats as engine_multi.hip's is and for its reason: the forward keeps
// 2 W floats of state and the own xdst pieces next to up to three loaded tiles per entry in flight, the column pass up to five.
// Entries in flight per slot (U): 4 in the forward (three loads per entry), 2 in the backward passes (four and five); UNTUNED -- chosen from
// the resource listing (profiles/spmm_gated_kernel_resources.txt): no scratch, no spills at any width.
constexpr int kMaxTile = 64;

template <int PASS>
void launch_pass(const sextans_engine *e, const sx::GatedArgs &a, const int *perm, hipStream_t s) {
    for_width(a.N < kMaxTile ? a.N : kMaxTile, [&](auto w) {
        using W = decltype(w);
        constexpr int U = PASS == sx::kAttnForward ? 4 : 2;
        if constexpr (4 * W::T * W::P <= kMaxTile) launch_pattern<sx::GatedPass<PASS, W::T, W::P, U>>(e, tiled<W>(a), perm, false, s);
    });
}

bool bad_mode(int mode) { return mode != SEXTANS_GATE_SUM && mode != SEXTANS_GATE_NORM; }
bool bad_eps(int mode, float eps) { return mode == SEXTANS_GATE_NORM && (!(eps > 0.0f) || std::isinf(eps)); }
// the operand struct: xdst, xsrc and V with their leading dimensions always, E's when it is given
bool bad_in(const sextans_gated_in *in, int N) {
    return bad_ld(in->ld_xdst, N) || bad_ld(in->ld_xsrc, N) || bad_ld(in->ld_v, N) || bad_ld_of(in->d_e, in->ld_e, N) ||
           misaligned(in->d_xdst, in->d_xsrc, in->d_v, in->d_e);
}

}  // namespace
}  // namespace sxe

using namespace sxe;

extern "C" {

int sextans_spmm_gated_device_rm(sextans_handle_t h, int mode, float eps, int N, const sextans_gated_in *in, float *d_C, int64_t ldc,
                                 float *d_den, int64_t ldden, float *d_z, int64_t ldz, void *stream) {
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
    sx::GatedArgs a{};
    a.xdst = in->d_xdst; a.xsrc = in->d_xsrc; a.V = in->d_v; a.E = in->d_e;
    a.ld_xdst = in->ld_xdst; a.ld_xsrc = in->ld_xsrc; a.ld_v = in->ld_v; a.ld_e = in->ld_e;
    a.out = d_C; a.den = d_den; a.z = d_z; a.ldc = ldc; a.ldden = ldden; a.ldz = ldz;
    a.norm = mode == SEXTANS_GATE_NORM; a.eps = eps; a.N = N;
    call.rows([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnForward>(e, a, perm, call.s); });
    return call.close("spmm_gated");
}

int64_t sextans_spmm_gated_workspace_floats(sextans_handle_t h, int mode, int N) {
    if (!h || bad_mode(mode) || bad_n(N) || too_many_tiles(N, kMaxTile)) return -(int64_t)SEXTANS_ERR_INVALID;
    if (!h->d_rp) return -(int64_t)SEXTANS_ERR_STATE;
    return mode == SEXTANS_GATE_NORM ? (int64_t)h->M * N : 0;
}

int sextans_spmm_gated_backward_device_rm(sextans_handle_t h, int mode, float eps, int N, const sextans_gated_in *in, const float *d_C, int64_t ldc,
                                          const float *d_den, int64_t ldden, const float *d_G, int64_t ldg, const float *d_Gz, int64_t ldgz,
                                          const sextans_gated_grad *out, float *d_work, void *stream) {
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
    sx::GatedArgs a{};
    a.xdst = in->d_xdst; a.xsrc = in->d_xsrc; a.V = in->d_v; a.E = in->d_e;
    a.ld_xdst = in->ld_xdst; a.ld_xsrc = in->ld_xsrc; a.ld_v = in->ld_v; a.ld_e = in->ld_e;
    a.C = d_C; a.ldc = ldc; a.Gz = d_Gz; a.ldgz = ldgz;
    a.gn = d_G; a.ldgn = ldg;
    a.dxdst = out->d_dxdst; a.dxsrc = out->d_dxsrc; a.dV = out->d_dv; a.dE = out->d_de;
    a.ld_dxdst = out->ld_dxdst; a.ld_dxsrc = out->ld_dxsrc; a.ld_dv = out->ld_dv; a.ld_de = out->ld_de;
    a.norm = norm; a.eps = eps; a.N = N;
    if (norm) {   // gn once, for both passes
        const long long items = (long long)h->M * (N / 4);
        hipLaunchKernelGGL(sx::gated_gn, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, call.s, (long long)h->M, N / 4, d_G, (long long)ldg,
                           d_den, (long long)ldden, eps, d_work);
        a.gn = d_work; a.ldgn = N;
    }
    if (cols) call.cols([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnBackwardCols>(e, a, perm, call.s); });
    if (rows) call.rows([&](const sextans_engine *e, const int *perm) { launch_pass<sx::kAttnBackwardRows>(e, a, perm, call.s); });
    return call.close("spmm_gated_backward");
}

}  // extern "C"
