// engine_launch.hip -- the launch layer (engine_launch.h): the only unit that instantiates the SpMM kernels.  A launcher computes the grid
// and the LDS bytes of ONE launch from the engine's state and turns options and widths into template arguments (dispatch.h); what is
// launched, in which order and on which operands is the routes' business.
#include <algorithm>

#include "chan_kernels.h"
#include "dispatch.h"
#include "engine_launch.h"
#include "reorder_kernels.h"
#include "spmm_bf16_kernels.h"
#include "spmm_colwise_kernel.h"
#include "spmm_csr_kernels.h"
#include "spmm_panel_v2.h"
#include "spmm_window_kernel.h"

static_assert(sxe::kBlock == sx::kBlock && sxe::kWideMaxDict == sx::kWideMaxDict, "engine_launch.h repeats two constants of the kernel headers");

namespace {
// 32 x 32 tiles through LDS: dst[c * ld_dst + r] = src[r * ld_src + c] for r < rows, c < cols (row-major -> column-major and back)
__global__ __launch_bounds__(256) void transpose_tiles(const float *__restrict__ src, int64_t ld_src, float *__restrict__ dst, int64_t ld_dst, int rows, int cols) {
    __shared__ float t[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8)
        if (r0 + i < rows && c0 + tx < cols) t[i][tx] = src[(int64_t)(r0 + i) * ld_src + c0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (c0 + i < cols && r0 + tx < rows) dst[(int64_t)(c0 + i) * ld_dst + r0 + tx] = t[tx][i];
}
// The same for the skinny matrices of the row-major fallback (rows x N, N a few tiles of 16): 64 rows x 16 columns per workgroup, the
// row-major side in 16-byte accesses (one wavefront = 16 rows x 64 bytes), the column-major side in 256-byte runs (one wavefront = 64
// consecutive rows of one column).  The row-major side must be 16-byte aligned with a leading dimension that is a multiple of 4.
template <bool TO_CM, int CW>   // TO_CM: rm[r * ld_rm + c] -> cm[c * ld_cm + r]; else the other way.  CW = 16 or 32 columns per workgroup
__global__ __launch_bounds__(256) void transpose_skinny(const float *__restrict__ src, float *__restrict__ dst, int64_t ld_rm, int64_t ld_cm, int rows, int cols) {
    // (CW = 32 from N = 32 on: the row-major side then moves whole 128-byte lines)
    __shared__ float t[CW][65];
    const int r0 = blockIdx.x * 64, c0 = blockIdx.y * CW, tid = threadIdx.x;
    constexpr int Q = CW / 4;                              // 16-byte pieces per row of the tile
    const int cc = tid >> 6, rc = tid & 63;               // column-major side: my column group (4 of them, Q columns each) and my row
    auto rm_side = [&](auto f) {
#pragma unroll
        for (int p = 0; p < 64 * Q / 256; ++p) {
            const int idx = tid + p * 256, rr = idx / Q, c4 = (idx % Q) * 4;
            if (r0 + rr < rows && c0 + c4 < cols) f(rr, c4);
        }
    };
    if constexpr (TO_CM) {
        rm_side([&](int rr, int c4) {
            const sx::f32x4 x = *reinterpret_cast<const sx::f32x4 *>(src + (int64_t)(r0 + rr) * ld_rm + c0 + c4);
            t[c4][rr] = x.x; t[c4 + 1][rr] = x.y; t[c4 + 2][rr] = x.z; t[c4 + 3][rr] = x.w;
        });
        __syncthreads();
        if (r0 + rc < rows)
#pragma unroll
            for (int i = 0; i < Q; ++i)
                if (c0 + cc * Q + i < cols) dst[(int64_t)(c0 + cc * Q + i) * ld_cm + r0 + rc] = t[cc * Q + i][rc];
    } else {
        if (r0 + rc < rows)
#pragma unroll
            for (int i = 0; i < Q; ++i)
                if (c0 + cc * Q + i < cols) t[cc * Q + i][rc] = src[(int64_t)(c0 + cc * Q + i) * ld_cm + r0 + rc];
        __syncthreads();
        rm_side([&](int rr, int c4) {
            *reinterpret_cast<sx::f32x4 *>(dst + (int64_t)(r0 + rr) * ld_rm + c0 + c4) = sx::f32x4{t[c4][rr], t[c4 + 1][rr], t[c4 + 2][rr], t[c4 + 3][rr]};
        });
    }
}
}  // namespace

namespace sxe {

void preload_device_code() {
    hipFuncAttributes fa;
    (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(&sx::repack_b_panels<16>));
    (void)hipGetLastError();
}

void launch_repack(int width, const float *dB, int64_t ldb, float *dBp, int K, int col_base, int ntiles, hipStream_t s, int k_begin,
                   int k_end, int ncols, const unsigned char *touched) {
    if (k_end < 0) k_end = K;
    if (k_end <= k_begin) return;
    if (ncols < 0) ncols = ntiles * width;
    dim3 grid((unsigned)((k_end - k_begin + sx::kBlock - 1) / sx::kBlock), (unsigned)ntiles);
    by_width(width, [&](auto L) {   // (panels of the segment's width: 4 * LPR columns)
        hipLaunchKernelGGL(sx::repack_b_panels<4 * decltype(L)::value>, grid, dim3(sx::kBlock), 0, s, dB, ldb, dBp, K, col_base, k_begin, k_end, ncols, touched);
    });
}

void launch_repack_perm(sextans_engine *h, const float *dB, int64_t ldb, float *dBp, int col_base, int ntiles, int ncols, hipStream_t s) {
    hipLaunchKernelGGL(sx::repack_b_panels_perm, dim3((unsigned)((h->col_hi - h->col_lo + sx::kBlock - 1) / sx::kBlock), (unsigned)ntiles), dim3(sx::kBlock), 0, s,
                       dB, ldb, dBp, h->K, col_base, h->cluster.d_colpos, h->col_lo, h->col_hi, ncols, h->mat.d_touched);
}

void launch_tiles_to_colmajor(const float *tiles, float *C, int64_t ldc, int M, int col0, int ntiles, int ncols, hipStream_t s) {
    hipLaunchKernelGGL(sx::tiles_to_colmajor, dim3((unsigned)((M + sx::kBlock - 1) / sx::kBlock), (unsigned)ntiles), dim3(sx::kBlock), 0, s, tiles, C, ldc, M, col0, ncols);
}

// What a kernel is told about B: floats between its panels of NT columns (kPanels), or the caller's leading dimension; the layout
// itself becomes the kernel's RM / BCOL template argument at the launch
static int64_t b_stride(const sextans_engine *h, const Operands &o, int NT) { return o.layout == BLayout::kPanels ? (int64_t)h->K * NT : o.ldb; }

void launch_rowgroup(sextans_engine *h, int width, const Operands &o, int ntiles, int row_end, const unsigned char *skip, const int *groups, int ngroups) {
    by_width(width, [&](auto L) {
        constexpr int LPR = decltype(L)::value, RB = sx::kBlock / LPR, CH = 2048;
        const int nrowblk = groups ? ngroups * std::max(1, 128 / RB) : (row_end - o.row_base + RB - 1) / RB;
        if (nrowblk <= 0) return;
        const unsigned nwg = (unsigned)nrowblk * (unsigned)ntiles;
        with_bool(h->opt_exact, [&](auto EX) { with_bool(h->opt_stage, [&](auto ST) { with_bool(o.layout == BLayout::kRowMajor, [&](auto RM) {
            hipLaunchKernelGGL((sx::spmm_csr_rowgroup<LPR, CH, decltype(EX)::value, decltype(ST)::value, decltype(RM)::value>), dim3(nwg), dim3(sx::kBlock), 0,
                               o.s, h->m_rp, h->m_rp + 1, h->m_ci, h->m_v, o.B, b_stride(h, o, 4 * LPR), o.C_in, o.ldc_in, o.C_out, o.ldc, o.row_base, row_end, ntiles, nrowblk,
                               o.alpha, o.beta, (int)h->opt_xcd, skip, groups);
        }); }); });
    });
}

int launch_panel(sextans_engine *h, int width, const Operands &o, int ntiles, int blk_begin, int blk_end) {
    const int nblk = blk_end - blk_begin;
    if (nblk <= 0) return SEXTANS_OK;
    if (int rc = restore_plan_streams(h)) return rc;   // (released while a clustered plan served the whole-matrix calls)
    by_width(width, [&](auto L) {
        constexpr int LPR = decltype(L)::value, RB = sx::kBlock / LPR, NT = 4 * LPR;
        const unsigned nwg = (unsigned)nblk * (unsigned)ntiles;
        const int xcd = (int)h->opt_xcd;
        // LDS = B panel sized for the largest dictionary of this matrix (rounded to 1 KiB) + C tile.
        const int pad_rows = h->ps.d_ioff ? sx::kWidePadRows : 1;   // (shared index lists may be shifted: their padding entries reach further)
        const int panel_floats = (h->ps.plan_pad_row + pad_rows) * NT;   // dictionary capacity + the +1.0f rows the padding entries address
        const int tile_floats = NT * (RB + 1);   // the C tile reuses the panel bytes
        const size_t lds = (size_t)(panel_floats > tile_floats ? panel_floats : tile_floats) * sizeof(int);
        auto go = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(nwg), dim3(sx::kBlock), lds, o.s, (const int2 *)h->ps.d_row_off.get(), h->ps.d_lidx,
                               h->ps.d_pcol32, h->ps.d_pval, h->ps.d_blk_row, h->ps.d_dict_ptr, h->ps.d_dict, h->ps.plan_dict_stride, o.B,
                               b_stride(h, o, NT), o.C_in, o.ldc_in, o.C_out, o.ldc, ntiles, nblk, o.alpha, o.beta, xcd, panel_floats,
                               (long long *)h->d_dbg.get(), blk_begin, o.row_base, (const unsigned char *)h->split.d_skip.get(), (const int2 *)h->ps.d_ioff.get(), pad_rows);
        };
        with_bool(h->opt_exact, [&](auto EX) {
            constexpr bool E = decltype(EX)::value;
            if (h->ps.plan_mixed) go(sx::spmm_csr_panel<LPR, E, true>);
            else if (o.layout == BLayout::kColMajor) go(sx::spmm_csr_panel<LPR, E, false, true>);
            else go(sx::spmm_csr_panel<LPR, E, false>);
        });
    });
    return SEXTANS_OK;
}

// ---- spmm_csr_panel_v2: what one launch is (V2Launch, decided by plan_panel_v2) and the instantiations that exist (PanelV2Kernels) ----------
namespace {
// Workgroup placement of the reordered form at N <= 32: false = row blocks to the XCDs round-robin (round 4, commit ad33d1a), true =
// contiguous chunks like every other launch.  Re-decided in round 5 with fabric traffic as a criterion: DESIGN 9 / profiles/r05_xcd_placement_ab.txt.
constexpr bool kReorderedContiguous = true;

struct V2Variant {   // the template arguments of spmm_csr_panel_v2 other than EXACT, with its defaults
    int H, NB; bool BCOL, TIMED = false; int DCAP = 9; bool CROW = false, BIG = false; int SETS = 1, RM = 0;
    bool operator==(const V2Variant &o) const {
        return H == o.H && NB == o.NB && BCOL == o.BCOL && TIMED == o.TIMED && DCAP == o.DCAP && CROW == o.CROW && BIG == o.BIG && SETS == o.SETS && RM == o.RM;
    }
};
struct V2Launch {   // everything decided for one launch
    int nb, tpw, ngrp, xcd;
    size_t lds;
    int64_t pstride;
    const int *dict, *slot_row;
    const unsigned char *skip;
    V2Variant v;
};

// the plan a launch walks
const sextans_engine::PanelState &v2_plan(const sextans_engine *h, V2Order order) { return order == V2Order::kNatural ? h->ps : h->cluster.psc; }

V2Launch plan_panel_v2(const sextans_engine *h, const Operands &o, int nsuper, int nblk, const PanelV2 &a) {
    V2Launch d{};
    const int H = a.H;
    const bool bcol = o.layout == BLayout::kColMajor, rm = o.layout == BLayout::kRowMajor;   // the kernel's BCOL and RM != 0
    const sextans_engine::PanelState &P = v2_plan(h, a.order);
    d.slot_row = (a.order == V2Order::kBricks || a.order == V2Order::kReordered) ? h->cluster.d_slot_row : nullptr;
    d.skip = a.order == V2Order::kPositions ? nullptr : (const unsigned char *)h->split.d_skip.get();   // rows on the piece path: never written by this kernel (kReordered: their staging rows keep C_in)
    const bool crow = a.order == V2Order::kReordered || a.order == V2Order::kPositions;
    // register-resident batches (16 entries each) per row: from the mean row length of the main matrix, so that matrices
    // with short rows (1-dof stencils: 27 entries) do not fetch six batches per row
    const int64_t mean_len = h->M > 0 ? h->m_nnz / h->M : 0;
    int nb = mean_len + 8 <= 32 ? 2 : mean_len + 8 <= 64 ? 4 : 6;
    {   // ... corrected by the longest row: no more batches than any row has, and one more when that makes EVERY row
        // register-resident (nasa4704: mean 22, longest 42 -- a quarter of the wavefronts otherwise finish a row from the
        // stream, one L2 round trip per 16 entries, and their workgroup waits for them)
        const int nb_max = std::max(1, (P.plan_max_row + 15) / 16);
        if (nb_max <= nb) nb = nb_max <= 2 ? 2 : nb_max <= 3 ? 3 : nb_max <= 4 ? 4 : 6;
        else if (nb == 2 && nb_max == 3) nb = 3;
    }
    d.nb = nb;
    const bool big = H == 1 && bcol && nb > 2;   // column-major staging + long rows: the 256-register form (2 workgroups per CU)
    int tpw = (int)h->opt_tiles_per_wg;
    if (tpw <= 0 && big) {   // ... in ONE round of workgroups
        tpw = std::min<int>(nsuper, std::max<int>(1, (int)(((int64_t)nblk * nsuper + 2 * h->num_cus - 1) / ((int64_t)2 * h->num_cus))));
    } else if (tpw <= 0 && rm && P.plan_sets == 2 && nsuper >= 4) {
        // row-major operands, two row sets per block (short-row 3-D grids), N >= 64: one tile per workgroup.  The workgroups of a block's
        // tiles are neighbours in the launch order, so the 64-byte halves of the B lines their panels are made of are asked for together,
        // and the panel copy is most of what such a block moves (3.4 dictionary rows per matrix row and tile against 26 entries once).
        // Same-box, 27-point 1-dof 4M rows: N = 64 / 128 / 256 0.459 / 0.389 / 0.335 -> 0.491 / 0.446 / 0.406 of the roofline; every other
        // class measured (long rows, one row set, column-major panels) loses 5 .. 20 % to the re-read of its entries
        // (profiles/r05_tiles_per_wg_ab.txt).
        tpw = 1;
    } else if (tpw <= 0) {   // all of N in one workgroup while that still leaves >= 4 rounds of workgroups (2 per CU)
        const int64_t rounds = (int64_t)nblk * nsuper / ((int64_t)8 * h->num_cus);
        tpw = (int)std::max<int64_t>(1, std::min<int64_t>(nsuper, rounds));
    }
    d.tpw = std::min(tpw, nsuper);
    d.ngrp = (nsuper + d.tpw - 1) / d.tpw;
    d.pstride = b_stride(h, o, 16);
    d.dict = (rm && crow && h->cluster.d_dict_nat) ? h->cluster.d_dict_nat : P.d_dict;
    // LDS = the panel: plan capacity + the +1.0f row.  A clustered plan of a short-row matrix is packed for a 320-row panel
    // (engine_plan.hip: small_panel): 20.5 KB instead of 36.9 KB per workgroup, so the CU holds as many workgroups as the registers
    // allow (5 at <= 96 registers) instead of the 4 the full panel permits -- these launches are latency-bound
    const bool small_panel = H == 1 && !bcol && P.plan_pad_row == 5 * 64;
    d.lds = small_panel ? (size_t)(5 * 64 + sx::kWidePadRows) * 64 : (size_t)H * sx::kWideHalfBytes;
    // contiguous chunks of row blocks per XCD -- except the reordered form at N <= 32, where handing the blocks of the merge-tree order to
    // the XCDs round-robin measured 1.3 .. 4.5 % faster (renumbered FEM 607 -> 582 us, unstructured mesh 444 -> 424; N = 128: +1.4 % the other way)
    // ("reordered_xcd": measurement switch for exactly this decision -- 0 round-robin, 1 contiguous chunks, -1 the rule above)
    d.xcd = crow && h->opt_reordered_xcd >= 0 ? (int)h->opt_reordered_xcd : (crow && nsuper <= 2 && !kReorderedContiguous) ? 0 : (int)h->opt_xcd;
    // ---- the variant ----
    V2Variant &v = d.v;
    if (H > 1) { v = {H, 6, bcol}; return d; }
    v = {1, nb, bcol};
    // small matrices staged from column-major B: dictionary capacity from the plan (5 x 64 covers nasa4704's 300)
    const bool small_dict = bcol && P.plan_max_dict <= 5 * 64 && h->opt_small_v2 != 0;
    if (h->opt_phase_timing && h->d_dbg && h->opt_exact && P.plan_sets == 1) {   // diagnostic instantiations: the forms the dispatcher uses most
        v.TIMED = true;
        if (small_dict && nb == 3) { v.DCAP = 5; return d; }
        if (bcol) { v.NB = 2; return d; }
        if (nb == 6 && !crow && !small_panel) return d;
        if (nb == 2 && !crow && small_panel) { v.DCAP = 5; return d; }
        v.TIMED = false;
    }
    if (small_dict) { v.NB = nb == 3 ? 3 : 2; v.DCAP = 5; }
    else if (big) { v.NB = nb <= 4 ? 4 : 6; v.BIG = true; }
    else if (bcol) v.NB = 2;
    else {
        // the caller's row-major operands: the 16-byte C accesses of the staging form on the caller's own rows, B without a repack
        // (C beyond 4 GB -- M * ldc * 4 bytes -- takes the instantiations with 64-bit lane addresses: RM == 2)
        if (rm) { v.CROW = true; v.RM = (int64_t)h->M * std::max(o.ldc, o.ldc_in) * 4 >= ((int64_t)1 << 32) ? 2 : 1; }
        else v.CROW = crow;   // block-major C staging
        // two row sets per block (short-row clustered plans: every row has <= 32 entries = 2 register-resident batches)
        if (P.plan_sets == 2) { v.NB = 2; v.SETS = 2; }
        else if (small_panel) { v.NB = nb >= 3 ? 3 : 2; v.DCAP = 5; }
    }
    return d;
}

// One legal combination of template arguments: every spmm_csr_panel_v2 the library holds is ONE entry of PanelV2Kernels below, times EXACT
// (the diagnostic TIMED forms: EXACT only).  A variant that is not listed is an error, never another kernel.
template <int H, int NB, bool BCOL, bool TIMED = false, int DCAP = 9, bool CROW = false, bool BIG = false, int SETS = 1, int RM = 0>
struct V2K {
    static constexpr V2Variant v{H, NB, BCOL, TIMED, DCAP, CROW, BIG, SETS, RM};
    template <class Go>
    static int launch(bool exact, Go &go) {
        if constexpr (TIMED) return go(sx::spmm_csr_panel_v2<H, NB, true, BCOL, TIMED, DCAP, CROW, BIG, SETS, RM>);
        else return with_bool(exact, [&](auto EX) { return go(sx::spmm_csr_panel_v2<H, NB, decltype(EX)::value, BCOL, TIMED, DCAP, CROW, BIG, SETS, RM>); });
    }
};
template <class... Ks>
struct V2List {
    template <class Go>
    static int launch(const V2Variant &v, bool exact, Go &go) {
        int rc = SEXTANS_ERR_STATE;
        const bool found = ((Ks::v == v ? (rc = Ks::launch(exact, go), true) : false) || ...);
        if (!found) g_last_error = "spmm_csr_panel_v2: no instantiation for the variant decided";
        return rc;
    }
};
template <int NB, int DCAP, int SETS, int RM>   // the caller's row-major operands; RM: 1 = 32-bit, 2 = 64-bit C addresses
using V2Rm = V2K<1, NB, false, false, DCAP, true, false, SETS, RM>;
using PanelV2Kernels = V2List<
    V2K<2, 6, true>, V2K<2, 6, false>,                                                                     // 32-column super tiles
    V2K<1, 3, true, true, 5>, V2K<1, 2, true, true>, V2K<1, 6, false, true>, V2K<1, 2, false, true, 5>,    // phase timing
    V2K<1, 3, true, false, 5>, V2K<1, 2, true, false, 5>,                                                  // column-major B, small dictionaries
    V2K<1, 4, true, false, 9, false, true>, V2K<1, 6, true, false, 9, false, true>,                        //   ... long rows: 256 registers
    V2K<1, 2, true>,                                                                                       //   ... otherwise
    V2Rm<2, 9, 2, 1>, V2Rm<3, 5, 1, 1>, V2Rm<2, 5, 1, 1>, V2Rm<2, 9, 1, 1>, V2Rm<3, 9, 1, 1>, V2Rm<4, 9, 1, 1>, V2Rm<6, 9, 1, 1>,
    V2Rm<2, 9, 2, 2>, V2Rm<3, 5, 1, 2>, V2Rm<2, 5, 1, 2>, V2Rm<2, 9, 1, 2>, V2Rm<3, 9, 1, 2>, V2Rm<4, 9, 1, 2>, V2Rm<6, 9, 1, 2>,
    V2K<1, 2, false, false, 9, true, false, 2>, V2K<1, 2, false, false, 9, false, false, 2>,               // two row sets, block-major C or not
    V2K<1, 3, false, false, 5, true>, V2K<1, 2, false, false, 5, true>,                                    // 320-row panel, block-major C
    V2K<1, 3, false, false, 5>, V2K<1, 2, false, false, 5>,                                                //   ... C in place
    V2K<1, 2, false, false, 9, true>, V2K<1, 3, false, false, 9, true>, V2K<1, 4, false, false, 9, true>, V2K<1, 6, false, false, 9, true>,
    V2K<1, 2, false>, V2K<1, 3, false>, V2K<1, 4, false>, V2K<1, 6, false>>;
}  // namespace

int launch_panel_v2(sextans_engine *h, const Operands &o, int nsuper, const PanelV2 &a) {
    const sextans_engine::PanelState &P = v2_plan(h, a.order);
    const int blk_end = a.blk_end < 0 ? P.plan_nblk : a.blk_end;
    const int nblk = a.dict_blocks_only ? P.n_dict_blocks : blk_end - a.blk_begin;
    if (nblk <= 0 || nsuper <= 0) return SEXTANS_OK;
    if (a.order == V2Order::kNatural)
        if (int rc = restore_plan_streams(h)) return rc;   // (released while a clustered plan served the whole-matrix calls)
    const V2Launch d = plan_panel_v2(h, o, nsuper, nblk, a);
    auto go = [&](auto kern) -> int {
        if (int rc = allow_big_lds(h, reinterpret_cast<const void *>(kern), (int)d.lds)) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)nblk * (unsigned)d.ngrp), dim3(sx::kBlock), d.lds, o.s, (const int2 *)P.d_row_off.get(),
                           P.d_lidx, P.d_pval, P.d_blk_row, P.d_dict_ptr, d.dict, P.plan_dict_stride, o.B, d.pstride, o.C_in, o.ldc_in, o.C_out, o.ldc, nsuper, d.tpw, nblk, o.alpha, o.beta, d.xcd,
                           P.plan_pad_row, a.blk_begin, o.row_base, d.skip, (long long *)h->d_dbg.get(), d.slot_row, (const int2 *)P.d_ioff.get(), a.last_cols, a.dict_blocks_only ? (const int *)P.d_dict_blocks.get() : (const int *)nullptr);
        return SEXTANS_OK;
    };
    return PanelV2Kernels::launch(d.v, h->opt_exact != 0, go);
}

namespace {
template <bool SCATTER>   // false: slab[t][i] = tiles[t][rows[i] - sub];  true: tiles[t][rows[i] - sub] = slab[t][i]   (16 floats each)
__global__ __launch_bounds__(256) void slab_rows(float *tiles, int64_t tile_stride, const int *__restrict__ rows, int sub, int n, float *slab, int64_t slab_stride) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(idx >> 2), q = (int)(idx & 3), t = blockIdx.y;
    if (i >= n) return;
    sx::f32x4 *a = reinterpret_cast<sx::f32x4 *>(tiles + (int64_t)t * tile_stride + (int64_t)(rows[i] - sub) * 16 + 4 * q);
    sx::f32x4 *b = reinterpret_cast<sx::f32x4 *>(slab + (int64_t)t * slab_stride + (int64_t)i * 16 + 4 * q);
    if (SCATTER) *a = *b; else *b = *a;
}
}  // namespace
void launch_slab_rows(bool scatter, float *tiles, int64_t tile_stride, const int *rows, int sub, int n, float *slab, int64_t slab_stride, int ntiles, hipStream_t s) {
    if (n <= 0) return;
    with_bool(scatter, [&](auto SC) {
        hipLaunchKernelGGL(slab_rows<decltype(SC)::value>, dim3((unsigned)(((int64_t)n * 4 + 255) / 256), (unsigned)ntiles), dim3(256), 0, s, tiles, tile_stride, rows, sub, n, slab, slab_stride);
    });
}

void launch_window(sextans_engine *h, const Operands &o, int ntiles, int wave_begin, int wave_end) {
    const int nwg = (wave_end - wave_begin + sx::kWinWaves - 1) / sx::kWinWaves;
    if (nwg <= 0) return;
    const size_t lds = (size_t)sx::kWinWaves * (size_t)(h->win.rw + 1) * sx::kWinNT * sizeof(float);
    with_bool(h->opt_exact, [&](auto EX) { with_value<4, 8>((int)h->opt_win_unroll, [&](auto U) {
        hipLaunchKernelGGL((sx::spmm_csr_window<decltype(EX)::value, decltype(U)::value>), dim3((unsigned)nwg * (unsigned)ntiles), dim3(sx::kWinWaves * 64), lds, o.s,
                           (const sx::u32x2 *)h->win.d_wstream.get(), (const int *)h->win.d_wstep0.get(), o.B, b_stride(h, o, sx::kWinNT), o.C_in,
                           o.ldc_in, o.C_out, o.ldc, h->M, h->win.rw, wave_begin, wave_end, nwg, o.row_base, o.alpha, o.beta, (const unsigned char *)h->split.d_skip.get());
    }); });
}

void launch_colwise(sextans_engine *h, const Operands &o, int N, int row_end) {
    const bool rm = o.layout == BLayout::kRowMajor;
    const int row_begin = o.row_base;
    const int64_t adjacent = h->opt_colwise_tiles_adjacent;
    auto tiles = [&](int width, int col0, int ntiles) {
        int T = 1, nrowblk, adj;
        if (rm) {
            // groups of T neighbouring lanes per row, one 16-column tile each (T = the largest divisor of the tile count up to 8): a
            // wavefront's loads cover T * 64 consecutive bytes of every row it touches
            if (adjacent != 0)
                for (int t = 8; t > 1; --t)
                    if (ntiles % t == 0) { T = t; break; }
            const int rows_per = sx::kBlock / T;
            nrowblk = (row_end - row_begin + rows_per - 1) / rows_per;
            adj = T == 1 && ntiles > 1 && adjacent != 0 && (int64_t)nrowblk * ntiles < ((int64_t)1 << 31) ? ntiles : 0;
        } else {
            // (tiles of a row block neighbours in the launch order: the row block's CSR entries come from HBM once -- measured on the 4M-row
            // 5-point stencil, two boxes: N = 32 0.513 / 0.527 -> 0.532 / 0.550 of the roofline; N = 48 / 64 equal or 1 % behind; N = 128 / 256
            // 0.51 -> 0.43 .. 0.49: more column streams in flight per XCD than its L2 keeps; "colwise_tiles_adjacent" 1 = two tiles, 2 = always,
            // 0 = never; profiles/r05_colwise_tile_order_ab.txt)
            nrowblk = (row_end - row_begin + sx::kBlock - 1) / sx::kBlock;
            adj = ntiles > 1 && (adjacent == 2 || (adjacent == 1 && ntiles <= 2)) && (int64_t)nrowblk * ntiles < ((int64_t)1 << 31) ? ntiles : 0;
        }
        const dim3 grid = adj ? dim3((unsigned)nrowblk * (unsigned)ntiles) : dim3((unsigned)nrowblk, (unsigned)(ntiles / T));
        with_bool(h->opt_exact, [&](auto EX) { with_value<16, 8>(width, [&](auto W) { with_bool(rm, [&](auto RM) {
            hipLaunchKernelGGL((sx::spmm_csr_colwise<decltype(EX)::value, decltype(W)::value, decltype(RM)::value>), grid, dim3(sx::kBlock), 0, o.s, h->m_rp, h->m_ci,
                               h->m_v, o.B, o.ldb, o.C_in, o.ldc_in, o.C_out, o.ldc, row_begin, row_end, nrowblk, col0, o.alpha, o.beta, (int)h->opt_xcd, (const unsigned char *)h->split.d_skip.get(), adj, T);
        }); }); });
    };
    const int n16 = N / 16;
    if (n16 > 0) tiles(16, 0, n16);
    if (N % 16) tiles(8, n16 * 16, 1);
}

void launch_chains(sextans_engine *h, const std::vector<Seg> &plan, const Operands &o, int c0, int c1, bool permuted_panels) {
    // row-major operands (sextans_spmm_device_rm): B is one "panel" with rows o.ldb floats apart
    const bool rm = o.layout == BLayout::kRowMajor;
    // permuted_panels (the reordered form): the 16-column panels hold B row k at row colpos[k]; the chain rows' entries come from
    // their compact relabelled copy (ensure_cluster_plan); 8-column remainder tiles keep the natural panels and the source arrays
    // one workgroup per (chain row, 16- or 8-column tile): chain_fused
    std::vector<Seg> segs;   // a segment whose last tile is half empty (N = 16 t + 8): its full tiles, then the 8 valid columns of the tail
    for (const Seg &g : plan) {
        if (g.last_cols == 8 && g.width == 16) {
            if (g.ntiles > 1) segs.push_back(Seg{16, g.col0, g.ntiles - 1, 0});
            segs.push_back(Seg{16, g.col0 + 16 * (g.ntiles - 1), 1, 8});
        } else {
            segs.push_back(g);
        }
    }
    for (const Seg &g : segs) {
        const float *bp = o.at(g.col0).B;
        const int NT = (g.width >= 16 && g.last_cols != 8) ? 16 : 8;   // (the tail: the first 8-column half of its 16-column panel)
        const int ntiles = g.last_cols == 8 ? 1 : g.ntiles * (g.width / NT);
        const bool perm = permuted_panels && g.width == 16;
        with_bool(h->opt_exact, [&](auto EX) { with_value<16, 8>(NT, [&](auto W) {
            constexpr int lds = sx::chain_fused_lds_bytes(decltype(W)::value), threads = sx::chain_fused_threads(decltype(W)::value);
            const auto kern = sx::chain_fused<decltype(W)::value, decltype(EX)::value>;
            (void)allow_big_lds(h, reinterpret_cast<const void *>(kern), lds);
            hipLaunchKernelGGL(kern, dim3((unsigned)(c1 - c0) * (unsigned)ntiles), dim3((unsigned)threads), (size_t)lds, o.s, h->split.d_chain_row,
                               perm ? h->cluster.d_chain_beg_c : h->split.d_chain_beg, h->split.d_chain_off, (c0 == 0 && c1 == h->split.nchain) ? h->split.d_chain_perm : (const int *)nullptr,
                               perm ? (const int *)h->cluster.d_chain_ci_perm : h->s_ci, perm ? (const float *)h->cluster.d_chain_v_c : h->s_v, bp, rm ? (int64_t)0 : (int64_t)h->K * g.width,
                               rm ? (int)o.ldb : g.width, o.C_in, o.ldc_in, o.C_out, o.ldc, g.col0, ntiles, c0, o.row_base, o.alpha, o.beta, rm ? 1 : 0);
        }); });
    }
}

void launch_hub_pieces(sextans_engine *h, int width, const sextans_engine::PieceTable &t, const Operands &o, int ntiles, int col0, int v0,
                       int v1, const int *colpos) {
    float *P = h->d_P + (int64_t)col0 * h->split.nv;
    by_width(width, [&](auto L) {
        constexpr int LPR = decltype(L)::value, RB = sx::kBlock / LPR;
        const int nblk = (v1 - v0 + RB - 1) / RB;
        if (nblk <= 0) return;
        with_bool(h->opt_exact, [&](auto EX) { with_bool(o.layout == BLayout::kRowMajor, [&](auto RM) {
            hipLaunchKernelGGL((sx::spmm_csr_pieces<LPR, decltype(EX)::value, decltype(RM)::value>), dim3((unsigned)nblk * (unsigned)ntiles), dim3(sx::kBlock), 0, o.s, t.d_vrp,
                               t.d_vend, h->s_ci, h->s_v, o.B, b_stride(h, o, 4 * LPR), P, (int64_t)h->split.nv, v0, v1, ntiles, colpos);
        }); });
    });
}

void launch_fold(sextans_engine *h, const sextans_engine::PieceTable &t, int hub0, int hub1, int N, const Operands &o) {
    const int64_t tot = (int64_t)(hub1 - hub0) * N;
    with_bool(h->opt_exact, [&](auto EX) {
        hipLaunchKernelGGL(sx::fold_hub_pieces<decltype(EX)::value>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, o.s, t.d_vfirst, t.d_row, h->d_P,
                           (int64_t)h->split.nv, o.C_in, o.ldc_in, o.C_out, o.ldc, hub0, hub1 - hub0, N, o.row_base, o.alpha, o.beta, o.c_rm ? 1 : 0);
    });
}

void launch_transpose(bool aligned, bool to_cm, const float *src, float *dst, int64_t ld_rm, int64_t ld_cm, int rows, int cols, hipStream_t s) {
    if (rows <= 0 || cols <= 0) return;
    if (!aligned) {   // transpose_tiles reads `rows x cols` row-major: the column-major side seen as cols x rows
        const int r = to_cm ? rows : cols, c = to_cm ? cols : rows;
        hipLaunchKernelGGL(transpose_tiles, dim3((unsigned)((c + 31) / 32), (unsigned)((r + 31) / 32)), dim3(256), 0, s, src, to_cm ? ld_rm : ld_cm, dst, to_cm ? ld_cm : ld_rm, r, c);
        return;
    }
    const int cw = cols >= 32 ? 32 : 16;
    const dim3 grid((unsigned)((rows + 63) / 64), (unsigned)((cols + cw - 1) / cw));
    with_bool(to_cm, [&](auto CM) { with_value<32, 16>(cw, [&](auto CW) {
        hipLaunchKernelGGL((transpose_skinny<decltype(CM)::value, decltype(CW)::value>), grid, dim3(256), 0, s, src, dst, ld_rm, ld_cm, rows, cols);
    }); });
}

// ---- bf16 dense operands (spmm_bf16_kernels.h) -----------------------------------------------------------------------------------
void launch_rowgroup_bf16(sextans_engine *h, int width, const OperandsBf16 &o, int ntiles) {
    by_width_bf16(width, [&](auto L) {
        constexpr int LPR = decltype(L)::value, RB = sx::kBlock / LPR, CH = 2048;
        const int nrowblk = (h->M + RB - 1) / RB;
        with_bool(h->opt_exact, [&](auto EX) { with_bool(h->opt_stage, [&](auto ST) { with_bool(o.c_elem == 2, [&](auto CB) {
            hipLaunchKernelGGL((sx::spmm_csr_rowgroup_bf16<LPR, CH, decltype(EX)::value, decltype(ST)::value, decltype(CB)::value>), dim3((unsigned)nrowblk * (unsigned)ntiles),
                               dim3(sx::kBlock), 0, o.s, h->m_rp, h->m_rp + 1, h->m_ci, h->m_v, o.B, o.ldb, (const void *)o.C_in, o.ldc_in, (void *)o.C_out, o.ldc, h->M, ntiles, nrowblk, o.alpha, o.beta,
                               (int)h->opt_xcd, (const unsigned char *)h->split.d_skip.get());
        }); }); });
    });
}

void launch_hub_pieces_bf16(sextans_engine *h, int width, const sextans_engine::PieceTable &t, const OperandsBf16 &o, int ntiles, int col0, int v0, int v1) {
    by_width_bf16(width, [&](auto L) {
        constexpr int LPR = decltype(L)::value, RB = sx::kBlock / LPR;
        const int nblk = (v1 - v0 + RB - 1) / RB;
        if (nblk <= 0) return;
        with_bool(h->opt_exact, [&](auto EX) {
            hipLaunchKernelGGL((sx::spmm_csr_pieces_bf16<LPR, decltype(EX)::value>), dim3((unsigned)nblk * (unsigned)ntiles), dim3(sx::kBlock), 0, o.s, t.d_vrp, t.d_vend,
                               h->s_ci, h->s_v, o.B, o.ldb, h->d_P + (int64_t)col0 * h->split.nv, (int64_t)h->split.nv, v0, v1, ntiles);
        });
    });
}

void launch_fold_bf16(sextans_engine *h, const sextans_engine::PieceTable &t, int N, const OperandsBf16 &o) {
    const int64_t tot = (int64_t)h->split.nhub * N;
    with_bool(h->opt_exact, [&](auto EX) {
        hipLaunchKernelGGL(sx::fold_hub_pieces_bf16<decltype(EX)::value>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, o.s, t.d_vfirst, t.d_row, h->d_P,
                           (int64_t)h->split.nv, (const uint16_t *)o.C_in, o.ldc_in, (uint16_t *)o.C_out, o.ldc, h->split.nhub, N, o.alpha, o.beta);
    });
}

void launch_widen(const uint16_t *src, int64_t lds, float *dst, int64_t ldd, int64_t rows, int cols, hipStream_t s) {
    if (rows <= 0) return;
    const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0 && lds % 8 == 0 && ldd % 4 == 0;
    const int64_t n = vec ? rows * (cols / 8) : rows * cols;
    with_bool(vec, [&](auto V) {
        hipLaunchKernelGGL(sx::widen_bf16_matrix<decltype(V)::value>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, lds, dst, ldd, rows, cols);
    });
}
void launch_round(const float *src, int64_t lds, uint16_t *dst, int64_t ldd, int64_t rows, int cols, hipStream_t s) {
    if (rows <= 0) return;
    const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0 && lds % 4 == 0 && ldd % 8 == 0;
    const int64_t n = vec ? rows * (cols / 8) : rows * cols;
    with_bool(vec, [&](auto V) {
        hipLaunchKernelGGL(sx::round_bf16_matrix<decltype(V)::value>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, lds, dst, ldd, rows, cols);
    });
}

void launch_chan_unpack_b(const float *ch, int64_t chan_len, int64_t colsize, int num_ch_b, int K, int N, float *B, hipStream_t s) {
    if (K > 0) sx::chan_unpack_b<<<dim3((unsigned)((K + 255) / 256), (unsigned)N), 256, 0, s>>>(ch, chan_len, colsize, num_ch_b, K, N, B);
}
void launch_chan_unpack_c(const float *ch, int64_t chan_len, int64_t colsize, int M, int N, float *C, hipStream_t s) {
    if (M > 0) sx::chan_unpack_c<<<dim3((unsigned)((M + 255) / 256), (unsigned)(N / 8)), 256, 0, s>>>(ch, chan_len, colsize, M, N, C);
}
void launch_chan_pack_c(const float *C, int M, int N, int64_t chan_len, int64_t colsize, float pad, float *ch, hipStream_t s) {
    if (colsize > 0) sx::chan_pack_c<<<dim3((unsigned)((colsize + 255) / 256), (unsigned)(N / 8)), 256, 0, s>>>(C, M, N, chan_len, colsize, pad, ch);
}

std::vector<Seg> widest_first(int N, int widest) {
    std::vector<Seg> v;
    int col = 0;
    if (N / widest) { v.push_back(Seg{widest, 0, N / widest}); col = N / widest * widest; }
    for (int w = widest / 2; w >= 8; w /= 2)
        if ((N - col) / w) { v.push_back(Seg{w, col, 1}); col += w; }
    return v;
}

const char *with_rowblocks(sextans_engine *h, const char *name) {
    h->last_kernel_buf = std::string(name) + "+rowblock_mfma_f32";
    return h->last_kernel_buf.c_str();
}
const char *kernel_name(MainKernel main, bool hubs, bool dense) {
    static const char *names[4][2][2] = {
        {{"spmm_csr_rowgroup", "spmm_csr_rowgroup+dense_tiles_mfma"},
         {"spmm_csr_rowgroup+hub_pieces", "spmm_csr_rowgroup+hub_pieces+dense_tiles_mfma"}},
        {{"spmm_csr_panel", "spmm_csr_panel+dense_tiles_mfma"},
         {"spmm_csr_panel+hub_pieces", "spmm_csr_panel+hub_pieces+dense_tiles_mfma"}},
        {{"spmm_csr_window", "spmm_csr_window+dense_tiles_mfma"},
         {"spmm_csr_window+hub_pieces", "spmm_csr_window+hub_pieces+dense_tiles_mfma"}},
        {{"spmm_csr_panel_v2", "spmm_csr_panel_v2+dense_tiles_mfma"},
         {"spmm_csr_panel_v2+hub_pieces", "spmm_csr_panel_v2+hub_pieces+dense_tiles_mfma"}}};
    return names[(int)main][hubs ? 1 : 0][dense ? 1 : 0];
}

}  // namespace sxe
