// engine_rowmajor.hip -- row-major operands: sextans_spmm_device_rm, its bf16 form and what prepares them.  The reference lays B and C
// out for its kernel on the host, OUTSIDE the timed call (sextans-host.cpp:150-195, 264-270); a caller whose operands are row-major (torch
// tensors; the natural layout of a "K x N feature matrix") gets the same here: no layout pass at all on the LDS-panel paths.
#include <algorithm>

#include "engine_launch.h"

using namespace sxe;

namespace {
__global__ __launch_bounds__(256) void invert_positions(int K, const int *__restrict__ colpos, int *__restrict__ colinv) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < K) colinv[colpos[k]] = k;
}
__global__ __launch_bounds__(256) void translate_dict(long long n, int K, const int *__restrict__ dict, const int *__restrict__ colinv, int *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { const int c = dict[i]; out[i] = (unsigned)c < (unsigned)K ? colinv[c] : 0; }   // (slots past a block's dictionary are never used)
}
}  // namespace
namespace sxe {
// Planning half of sextans_spmm_device_rm: everything that allocates, builds or synchronises with the host -- the lean prepare(), the
// reconsideration of a clustered plan declined for column-major calls only, and the clustered plan's dictionaries translated back to
// the caller's column numbers.  Run by the first row-major call, or ahead of it by sextans_prepare / sextans_dist_prepare so that no
// timed (or captured) call builds anything.
int rm_plan(sextans_engine *h, int N, hipStream_t s, Tiling *out) {
    // (N = 8 runs as one half-empty 16-column tile of the 16-column plan: without a repack to pay for there is no reason for a second
    // packed plan at 2 lanes per row)
    const int Nplan = N == 8 ? 16 : N;
    // (no B-panel / C-staging workspaces on behalf of this call: 8 GB each at K = M = 4M, N = 512, for paths that repack and stage nothing;
    // the fallback at the end plans again through the column-major entry and gets them)
    struct Lean { sextans_engine *h; ~Lean() { h->lean_prepare = false; } } lean{h};
    h->lean_prepare = true;
    Tiling t;
    if (int rc = prepare(h, Nplan, true, &t)) return rc;
    // A clustered plan that was declined only because the column-major form has to pay two passes over C for it (decline 12) is
    // reconsidered for this layout, where it costs nothing: built once, used by row-major calls only unless it pays for both.
    if ((h->cluster.state == -1 || h->cluster.runs) && h->cluster.decline == 12 && !h->cluster_rm_tried && t.W == 16 && h->opt_row_cluster < 0) {
        h->cluster_rm_tried = true;
        free_cluster_plan(h);
        h->cluster_for_rm = true;
        const int rc = prepare(h, Nplan, true, &t);
        h->cluster_for_rm = false;
        if (rc) return rc;
    }
    if (t.W == 16 && h->cluster.state == 2 && h->cluster.d_colpos && !h->cluster.d_dict_nat) {   // the plan's dictionaries hold relabelled columns: translate them back once
        const long long n = (long long)h->cluster.psc.plan_nblk * h->cluster.psc.plan_dict_stride;
        DevBuf<int> colinv;
        if (colinv.alloc((size_t)std::max(h->K, 1)) != hipSuccess || h->cluster.d_dict_nat.alloc((size_t)std::max<long long>(n, 1)) != hipSuccess) {
            (void)hipGetLastError();
            g_last_error = "row-major plan: out of device memory for the translated block dictionaries";
            return SEXTANS_ERR_HIP;
        }
        hipLaunchKernelGGL(invert_positions, dim3((unsigned)((h->K + 255) / 256)), dim3(256), 0, s, h->K, h->cluster.d_colpos, colinv);
        hipLaunchKernelGGL(translate_dict, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, h->K, h->cluster.psc.d_dict, colinv, h->cluster.d_dict_nat);
        SX_HIP(hipStreamSynchronize(s));
    }
    if (out) *out = std::move(t);
    return SEXTANS_OK;
}
int check_rm_bf16_args(sextans_handle_t h, int N, const uint16_t *d_B, int64_t ldb, const void *d_C_in, int64_t ldc_in, void *d_C_out, int64_t ldc, int c_dtype) {
    if (!h || N <= 0 || (N % 8) != 0 || !d_B || !d_C_in || !d_C_out || ldb < N || ldc_in < N || ldc < N) return SEXTANS_ERR_INVALID;
    if (c_dtype != SEXTANS_DTYPE_F32 && c_dtype != SEXTANS_DTYPE_BF16) return SEXTANS_ERR_INVALID;
    const uintptr_t cmask = c_dtype == SEXTANS_DTYPE_BF16 ? 1 : 3;   // addresses that cannot hold an element of their type
    if ((reinterpret_cast<uintptr_t>(d_B) & 1) || ((reinterpret_cast<uintptr_t>(d_C_in) | reinterpret_cast<uintptr_t>(d_C_out)) & cmask)) return SEXTANS_ERR_INVALID;
    return SEXTANS_OK;
}
}  // namespace sxe
namespace {
// Everything sextans_spmm_device_rm decides for one call (route_rm), before anything is launched
struct RouteRM {
    enum Path { kColwise, kPanelV2, kRowgroup, kTranspose } path = kTranspose;
    bool aligned = false;        // 16-byte accesses on the caller's operands (rm_aligned, bf16_aligned)
    V2Order order = V2Order::kNatural;   // kPanelV2: the plan launch_panel_v2 walks
    bool split = false;          // kPanelV2 on a mixed plan: dictionary blocks there, the other blocks' rows on the gather kernel
    std::vector<Seg> segs;       // kRowgroup: the tiling of N
};

// fp32 operands: 16-byte aligned with leading dimensions that are multiples of 4
bool rm_aligned(const Operands &o) {
    return ((reinterpret_cast<uintptr_t>(o.B) | reinterpret_cast<uintptr_t>(o.C_in) | reinterpret_cast<uintptr_t>(o.C_out)) & 15) == 0 && o.ldb % 4 == 0 &&
           o.ldc_in % 4 == 0 && o.ldc % 4 == 0;
}

// Asked with what it reads of the operands: the alignment verdict, B's leading dimension (in floats) and N
RouteRM route_rm(const sextans_engine *h, const Tiling &t, bool aligned, int64_t ldb, int N) {
    RouteRM r;
    const bool colwise = colwise_wanted(h);
    r.aligned = aligned;
    // 32-bit offsets inside the kernel: floats into B (C beyond 4 GB: the kernel's 64-bit form, launch_panel_v2)
    const bool fits = (int64_t)h->K * ldb < ((int64_t)1 << 32);
    // Rows on the long-row paths (pieces, exact chains): from the caller's row-major B into its row-major C as well -- the piece kernel's
    // 16-byte gathers and the chain producers' LDS-DMA read B rows ldb floats apart instead of panel rows, the fold and the chain
    // consumer write C[r * ldc + n].  The main kernels skip those rows (d_skip), so the order between the launches does not matter;
    // the chains run beside the main kernel on the engine's side stream, as in the column-major form.
    const bool hubs = h->split.nhub > 0, chains = h->split.nchain > 0;
    const bool long_ok = (!hubs && !chains) || (r.aligned && (!chains || (h->aux_stream && h->ev_fork && h->ev_join && ldb < ((int64_t)1 << 31))));
    if (colwise && r.aligned && !hubs && !chains && csr_only(h) && h->m_nnz > 0) {   // short rows in a local numbering: lane per row, 16-byte accesses
        r.path = RouteRM::kColwise;
        return r;
    }
    if (t.W == 16 && (h->opt_kernel == 0 || h->opt_kernel == 2) && h->opt_panel_v2 != 0 && h->opt_cols_per_lane != 8 && csr_only(h) &&
        !(colwise && !hubs && !chains) && r.aligned && fits && long_ok && h->m_nnz > 0) {
        if (h->cluster.state == 2) { r.order = V2Order::kReordered; r.path = RouteRM::kPanelV2; }
        else if (h->cluster.state == 1) { r.order = V2Order::kBricks; r.path = RouteRM::kPanelV2; }
        else if (t.panel && (!h->ps.plan_mixed || (h->ps.d_rg_skip && h->opt_split_mixed != 0 && h->opt_kernel == 0)) && h->ps.plan_max_dict <= kWideMaxDict) r.path = RouteRM::kPanelV2;
    }
    if (r.order == V2Order::kReordered && h->cluster.d_colpos && !h->cluster.d_dict_nat) r.path = RouteRM::kTranspose;   // (cannot happen after rm_plan; kept as a guard)
    if (r.path == RouteRM::kPanelV2) {
        r.split = r.order == V2Order::kNatural && h->ps.plan_mixed;
        return r;
    }
    // The gather kernel on a matrix without rows on the piece / chain / dense-tile paths: a row of row-major B IS what its lanes fetch
    // per non-zero (the 4 * LPR floats of a panel row), and a lane's 4 accumulators are 16 bytes of its C row -- no repack, no passes.
    if (!t.panel && !t.window && !(colwise && !hubs && !chains) && r.aligned && long_ok && (h->opt_kernel == 0 || h->opt_kernel == 1) && csr_only(h) && h->m_nnz > 0) {
        r.path = RouteRM::kRowgroup;
        r.segs = t.segs;
        if (N == 8) r.segs.assign(1, Seg{8, 0, 1});   // (the plan above was made for 16 columns)
        return r;
    }
    // Everything else (lane-per-row / window kernels, mixed plans, rows on the piece and chain paths, dense tiles, unaligned operands):
    // through column-major copies in the engine's workspaces
    return r;
}

int run_rm_colwise(sextans_engine *h, const Call &c) {
    Prof p(h, &h->ev_kernel, c.o.s);
    launch_colwise(h, c.o, c.N, h->M);
    h->last_kernel = "spmm_csr_colwise_rowmajor";
    SX_HIP(hipGetLastError());
    return SEXTANS_OK;
}

// The paths on the caller's row-major operands (kPanelV2, kRowgroup), rows on the long-row paths included
int run_rm_direct(sextans_engine *h, const Call &c, const RouteRM &r) {
    Prof p(h, &h->ev_kernel, c.o.s);
    const bool long_rows = h->split.nhub > 0 || h->split.nchain > 0;
    if (h->split.nchain > 0) {
        std::vector<Seg> segs;   // tiles of the chain kernel: 16-column tiles and an 8-column tail (never past column N of a B row)
        if (c.N / 16) segs.push_back(Seg{16, 0, c.N / 16});
        if (c.N % 16) segs.push_back(Seg{8, c.N / 16 * 16, 1});
        if (int rc = fork_chains(h, c.o, segs, 0, h->split.nchain)) return rc;
    }
    // the gather kernel: over the rows of the blocks without a dictionary (split form of a mixed plan), or over all rows
    auto rowgroups = [&](const std::vector<Seg> &segs, const unsigned char *skip, const int *groups, int ngroups) {
        for (const Seg &g : segs) launch_rowgroup(h, g.width, c.o.at(g.col0), g.ntiles, h->M, skip, groups, ngroups);
    };
    if (r.path == RouteRM::kPanelV2) {
        PanelV2 a;
        a.order = r.order;
        a.last_cols = c.N % 16 ? 8 : 16;
        a.dict_blocks_only = r.split;
        if (int rc = launch_panel_v2(h, c.o, (c.N + 15) / 16, a)) return rc;
        if (r.split) rowgroups(wide_first(c.N), h->ps.d_rg_skip, h->ps.d_rg_groups, h->ps.rg_ngroups);
    } else {
        rowgroups(r.segs, h->split.d_skip, nullptr, 0);
    }
    if (h->split.nhub > 0) {   // the long rows' pieces and their fold
        const sextans_engine::PieceTable &pt = h->split.by_len;
        const int v0 = pt.h_vfirst[0], v1 = pt.h_vfirst[(size_t)h->split.nhub];
        for (const Seg &g : wide_first(c.N)) launch_hub_pieces(h, g.width, pt, c.o.at(g.col0), g.ntiles, g.col0, v0, v1);
        launch_fold(h, pt, 0, h->split.nhub, c.N, c.o);
    }
    if (h->split.nchain > 0) SX_HIP(hipStreamWaitEvent(c.o.s, h->ev_join, 0));
    h->last_kernel = r.path == RouteRM::kRowgroup ? (long_rows ? "spmm_csr_rowgroup_rowmajor+long_rows" : "spmm_csr_rowgroup_rowmajor")
                     : r.order == V2Order::kReordered ? (long_rows ? "spmm_csr_panel_v2_rowmajor_clustered+long_rows" : "spmm_csr_panel_v2_rowmajor_clustered")
                                                      : (long_rows ? "spmm_csr_panel_v2_rowmajor+long_rows" : "spmm_csr_panel_v2_rowmajor");
    SX_HIP(hipGetLastError());
    return SEXTANS_OK;
}

// Column-major copies in the engine's workspaces -- two transposes in front, one behind -- around the column-major entry point.
// (workspaces of their own -- not the host-buffer entry points' d_B / d_Cin / d_Cout, which are filled on another stream; C_in and
// C_out may alias, so one C buffer)
int run_rm_transpose(sextans_engine *h, const Call &c, bool aligned) {
    const int N = c.N;
    const Operands &o = c.o;
    h->lean_prepare = false;
    const size_t nB = (size_t)h->K * (size_t)N, nC = (size_t)h->M * (size_t)N;
    if (int rc = reserve(h->d_rmB, nB)) return rc;
    if (int rc = reserve(h->d_rmC, nC)) return rc;
    {
        Prof p(h, &h->ev_repack, o.s);
        launch_transpose(aligned, true, o.B, h->d_rmB, o.ldb, h->K, h->K, N, o.s);
        launch_transpose(aligned, true, o.C_in, h->d_rmC, o.ldc_in, h->M, h->M, N, o.s);
    }
    if (int rc = sextans_spmm_device_rows(h, N, o.alpha, h->d_rmB, h->K, o.beta, h->d_rmC, h->M, h->d_rmC, h->M, 0, h->M, 0, (void *)o.s)) return rc;
    {
        Prof p(h, &h->ev_post, o.s);
        launch_transpose(aligned, false, h->d_rmC, o.C_out, o.ldc, h->M, h->M, N, o.s);
    }
    SX_HIP(hipGetLastError());
    return SEXTANS_OK;
}

// ---- bf16 dense operands on the row-major entry (spmm_bf16_kernels.h) --------------------------------------------------------------
struct CallBf16 {   // o.C_in / o.C_out in bytes, o.c_elem bytes per element
    OperandsBf16 o; int N = 0;
    bool cbf16() const { return o.c_elem == 2; }
};

// The native route: the gather kernel (and the piece path of long rows) on the caller's bf16 buffers.  The very arrays run_rm_direct
// passes (m_rp / m_ci / m_v, the piece table by_len) -- what a value refresh rewrites.
int run_rm_bf16_native(sextans_engine *h, const CallBf16 &c) {
    const OperandsBf16 &o = c.o;
    Prof p(h, &h->ev_kernel, o.s);
    for (const Seg &g : bf16_tiles(c.N)) launch_rowgroup_bf16(h, g.width, o.at(g.col0), g.ntiles);
    if (h->split.nhub > 0) {   // the long rows' pieces (raw fp32 sums into P) and their fold
        const sextans_engine::PieceTable &pt = h->split.by_len;
        const int v0 = pt.h_vfirst[0], v1 = pt.h_vfirst[(size_t)h->split.nhub];
        for (const Seg &g : bf16_tiles(c.N)) launch_hub_pieces_bf16(h, g.width, pt, o.at(g.col0), g.ntiles, g.col0, v0, v1);
        if (c.cbf16()) {
            launch_fold_bf16(h, pt, c.N, o);
        } else {   // fp32 C: the fold of the fp32 route
            Operands f;
            f.C_in = (const float *)o.C_in; f.ldc_in = o.ldc_in; f.C_out = (float *)o.C_out; f.ldc = o.ldc; f.c_rm = true;
            f.alpha = o.alpha; f.beta = o.beta; f.s = o.s;
            launch_fold(h, pt, 0, h->split.nhub, c.N, f);
        }
    }
    h->last_kernel = h->split.nhub > 0 ? "spmm_csr_rowgroup_rowmajor_bf16+long_rows" : "spmm_csr_rowgroup_rowmajor_bf16";
    SX_HIP(hipGetLastError());
    ++h->mat.bf16_native_calls;
    return SEXTANS_OK;
}

// the converting route's fp32 copies: B always, C only when it is bf16
int ensure_bf16_workspaces(sextans_engine *h, int N, bool cbf16) {
    if (int rc = reserve(h->mat.d_bfB, (size_t)h->K * (size_t)N)) return rc;
    if (cbf16)
        if (int rc = reserve(h->mat.d_bfC, (size_t)h->M * (size_t)N)) return rc;
    return SEXTANS_OK;
}

// Every other route: fp32 copies of B (and of a bf16 C) in the engine's workspaces around the fp32 row-major entry point
int run_rm_bf16_converted(sextans_engine *h, const CallBf16 &c) {
    const OperandsBf16 &o = c.o;
    const int N = c.N;
    if (int rc = ensure_bf16_workspaces(h, N, c.cbf16())) return rc;
    {
        Prof p(h, &h->ev_repack, o.s);
        launch_widen(o.B, o.ldb, h->mat.d_bfB, N, h->K, N, o.s);
        if (c.cbf16()) launch_widen((const uint16_t *)o.C_in, o.ldc_in, h->mat.d_bfC, N, h->M, N, o.s);
    }
    SX_HIP(hipGetLastError());
    if (!c.cbf16()) {
        if (int rc = sextans_spmm_device_rm(h, N, o.alpha, h->mat.d_bfB, N, o.beta, (const float *)o.C_in, o.ldc_in, (float *)o.C_out, o.ldc, (void *)o.s)) return rc;
    } else {
        if (int rc = sextans_spmm_device_rm(h, N, o.alpha, h->mat.d_bfB, N, o.beta, h->mat.d_bfC, N, h->mat.d_bfC, N, (void *)o.s)) return rc;
        Prof p(h, &h->ev_post, o.s);
        launch_round(h->mat.d_bfC, N, (uint16_t *)o.C_out, o.ldc, h->M, N, o.s);
    }
    SX_HIP(hipGetLastError());
    ++h->mat.bf16_converted_calls;
    return SEXTANS_OK;
}

// 16-byte accesses on the caller's buffers: aligned bases, whole 16-byte groups per row; 32-bit byte offsets into B
bool bf16_aligned(const sextans_engine *h, const OperandsBf16 &o) {
    const int64_t cm = 16 / o.c_elem;
    return (int64_t)h->K * o.ldb * 2 < ((int64_t)1 << 32) && ((reinterpret_cast<uintptr_t>(o.B) | reinterpret_cast<uintptr_t>(o.C_in) | reinterpret_cast<uintptr_t>(o.C_out)) & 15) == 0 &&
           o.ldb % 8 == 0 && o.ldc_in % cm == 0 && o.ldc % cm == 0;
}
// route_rm's decision for the call, unchanged: native where it is the gather kernel and no row is an exact chain
// (asked with the caller's leading dimension; a call that converts asks again inside sextans_spmm_device_rm with ldb = N of the
// workspace -- route_rm looks at ldb only for the 32-bit limit of the panel paths, so the two cannot disagree on the gather route;
// operands that pass bf16_aligned are aligned in route_rm's sense too)
bool bf16_native(const sextans_engine *h, const CallBf16 &c, const Tiling &t) {
    if (!bf16_aligned(h, c.o) || h->split.nchain > 0) return false;
    return route_rm(h, t, true, c.o.ldb, c.N).path == RouteRM::kRowgroup;
}
// the bf16 entry points' operands (C addressed in bytes)
CallBf16 bf16_call(int N, float alpha, const uint16_t *d_B, int64_t ldb, float beta, const void *d_C_in, int64_t ldc_in, void *d_C_out, int64_t ldc, int c_dtype, hipStream_t s) {
    CallBf16 c;
    c.N = N;
    c.o.B = d_B; c.o.ldb = ldb; c.o.layout = BLayout::kRowMajor;
    c.o.C_in = (const char *)d_C_in; c.o.ldc_in = ldc_in; c.o.C_out = (char *)d_C_out; c.o.ldc = ldc; c.o.c_rm = true;
    c.o.c_elem = c_dtype == SEXTANS_DTYPE_BF16 ? 2 : 4; c.o.alpha = alpha; c.o.beta = beta; c.o.s = s;
    return c;
}
}  // namespace
extern "C" {

int sextans_prepare(sextans_handle_t h, int N, int layout, void *stream) {
    if (!h || N <= 0 || (N % 8) != 0 || (layout != SEXTANS_LAYOUT_COLMAJOR && layout != SEXTANS_LAYOUT_ROWMAJOR && layout != SEXTANS_LAYOUT_ROWMAJOR_T))
        return SEXTANS_ERR_INVALID;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    SX_HIP(hipSetDevice(h->device));
    if (layout == SEXTANS_LAYOUT_ROWMAJOR_T) return prepare_transposed(h, N, (hipStream_t)stream);
    if (h->M == 0) return SEXTANS_OK;
    if (layout == SEXTANS_LAYOUT_ROWMAJOR) return rm_plan(h, N, (hipStream_t)stream);
    return prepare(h, N);
}

int sextans_spmm_device_rm(sextans_handle_t h, int N, float alpha, const float *d_B, int64_t ldb, float beta, const float *d_C_in,
                           int64_t ldc_in, float *d_C_out, int64_t ldc, void *stream) {
    if (!h || N <= 0 || (N % 8) != 0 || !d_B || !d_C_in || !d_C_out || ldb < N || ldc_in < N || ldc < N) return SEXTANS_ERR_INVALID;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    SX_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (h->M == 0) return SEXTANS_OK;
    Tiling t;
    if (int rc = rm_plan(h, N, s, &t)) return rc;
    Call c;
    c.N = N; c.row_end = h->M;
    c.o.B = d_B; c.o.ldb = ldb; c.o.layout = BLayout::kRowMajor;
    c.o.C_in = d_C_in; c.o.ldc_in = ldc_in; c.o.C_out = d_C_out; c.o.ldc = ldc; c.o.c_rm = true;
    c.o.alpha = alpha; c.o.beta = beta; c.o.s = s;
    const RouteRM r = route_rm(h, t, rm_aligned(c.o), ldb, N);
    switch (r.path) {
        case RouteRM::kColwise: return run_rm_colwise(h, c);
        case RouteRM::kTranspose: return run_rm_transpose(h, c, r.aligned);
        default: return run_rm_direct(h, c, r);
    }
}

int sextans_spmm_device_rm_bf16(sextans_handle_t h, int N, float alpha, const uint16_t *d_B, int64_t ldb, float beta, const void *d_C_in,
                                int64_t ldc_in, void *d_C_out, int64_t ldc, int c_dtype, void *stream) {
    if (int rc = check_rm_bf16_args(h, N, d_B, ldb, d_C_in, ldc_in, d_C_out, ldc, c_dtype)) return rc;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    SX_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (h->M == 0) return SEXTANS_OK;
    Tiling t;
    if (int rc = rm_plan(h, N, s, &t)) return rc;
    const CallBf16 c = bf16_call(N, alpha, d_B, ldb, beta, d_C_in, ldc_in, d_C_out, ldc, c_dtype, s);
    return bf16_native(h, c, t) ? run_rm_bf16_native(h, c) : run_rm_bf16_converted(h, c);
}

int sextans_prepare_rm_bf16(sextans_handle_t h, int N, int c_dtype, int transposed, void *stream) {
    if (!h || N <= 0 || (N % 8) != 0 || (c_dtype != SEXTANS_DTYPE_F32 && c_dtype != SEXTANS_DTYPE_BF16) || (transposed != 0 && transposed != 1))
        return SEXTANS_ERR_INVALID;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    SX_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (transposed) {
        if (int rc = prepare_transposed(h, N, s)) return rc;
        return h->tr ? sextans_prepare_rm_bf16(h->tr, N, c_dtype, 0, stream) : SEXTANS_OK;
    }
    if (h->M == 0) return SEXTANS_OK;
    Tiling t;
    if (int rc = rm_plan(h, N, s, &t)) return rc;
    // the route of a call with aligned operands; where that is native nothing more is needed (a call with unaligned operands on such a
    // matrix converts and sizes the copies itself)
    const CallBf16 c = bf16_call(N, 1.f, nullptr, N, 0.f, nullptr, N, nullptr, N, c_dtype, s);
    if (bf16_native(h, c, t)) return SEXTANS_OK;
    return ensure_bf16_workspaces(h, N, c.cbf16());
}

}  // extern "C"
