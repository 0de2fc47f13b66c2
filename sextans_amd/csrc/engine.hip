// engine.hip -- the SpMM engine behind the C ABI (include/sextans_amd.h): replaces the
// tapa::invoke(Sextans, ...) boundary of the reference (sextans-host.cpp:237-251, sextans.h:20-26).
//
// One engine = one HIP device.  The CSR arrays are uploaded once (sextans_set_matrix_csr).  The first SpMM on a
// matrix (or sextans_align_row / sextans_get_stat) prepares it on the host, outside every timed region like the
// reference's scheduling and packing (sextans-host.cpp:114-148): matrix as set -> [dense 32x32 tiles to bf16 MFMA,
// opt-in] -> source -> [long rows to the piece path] -> main matrix -> packed row-bucketed form (LDS-panel kernel)
// where row blocks reuse B rows.  Every spmm call then enqueues on the caller's stream, without host
// synchronisation in the device-resident form: (1) B repack column-major -> N-tile panels, (2) the main kernel
// (row-group gather / LDS panel / K-window sweep) [+ MFMA pass over the dense tiles, + piece kernel and in-order
// fold for long rows], (3) for the multi-GPU entry the RCCL all-gather of the C slabs, chunk-pipelined.
// There is NO CPU fallback anywhere in this file: no device => SEXTANS_ERR_NO_DEVICE.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "chan_kernels.h"
#include "engine_state.h"
#include "reorder_kernels.h"
#include "spmm_colwise_kernel.h"
#include "spmm_bf16_kernels.h"
#include "spmm_csr_kernels.h"
#include "spmm_panel_v2.h"
#include "spmm_window_kernel.h"
#include "window_plan.h"

namespace sxe {
thread_local std::string g_last_error;
}
using namespace sxe;

namespace sxe {

int check_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        g_last_error = "hipGetDeviceCount: no HIP device";
        return SEXTANS_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) return SEXTANS_ERR_INVALID;
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device) != hipSuccess) return SEXTANS_ERR_NO_DEVICE;
    if (strncmp(p.gcnArchName, "gfx950", 6) != 0) {
        g_last_error = std::string("device is ") + p.gcnArchName + ", engine is built for gfx950 only";
        return SEXTANS_ERR_NO_DEVICE;
    }
    return SEXTANS_OK;
}

template <int W>
void launch_repack(const float *dB, int64_t ldb, float *dBp, int K, int col_base, int ntiles,
                   hipStream_t s, int k_begin = 0, int k_end = -1, int ncols = -1, const unsigned char *touched = nullptr) {
    if (k_end < 0) k_end = K;
    if (k_end <= k_begin) return;
    if (ncols < 0) ncols = ntiles * W;   // (fewer: the last panel is zero-filled past them)
    dim3 grid((unsigned)((k_end - k_begin + sx::kBlock - 1) / sx::kBlock), (unsigned)ntiles);
    hipLaunchKernelGGL(sx::repack_b_panels<W>, grid, dim3(sx::kBlock), 0, s, dB, ldb, dBp, K,
                       col_base, k_begin, k_end, ncols, touched);
}

template <int LPR>
void launch_rowgroup(sextans_engine *h, const int *rp, const int *rend, const int *ci, const float *va, bool pieces,
                     const unsigned char *skip, const float *dBp,
                     const float *dCin, int64_t ldc_in, float *dCout, int64_t ldc, int row_begin, int row_end, int ntiles,
                     float alpha, float beta, hipStream_t s, int64_t rm_ldb = 0, bool round_robin = false, const int *groups = nullptr, int ngroups = 0) {
    // groups: the launch covers only these groups of 128 rows (row_begin must be 0)
    // rm_ldb > 0: dBp / dCin / dCout are the caller's ROW-major operands at this segment's first column (sextans_spmm_device_rm)
    // round_robin: workgroups to the XCDs in launch order (the split form of a mixed plan: most workgroups leave at once, and contiguous
    // chunks per XCD would put all the working ones on one or two XCDs)
    constexpr int RB = sx::kBlock / LPR;
    constexpr int CH = 2048;
    const int nrowblk = groups ? ngroups * std::max(1, 128 / RB) : (row_end - row_begin + RB - 1) / RB;
    if (nrowblk <= 0) return;
    const unsigned nwg = (unsigned)nrowblk * (unsigned)ntiles;
    const int64_t pstride = rm_ldb > 0 ? rm_ldb : (int64_t)h->K * 4 * LPR;
    const int xcd = round_robin ? 0 : (int)h->opt_xcd;
#define SX_LAUNCH(EX, ST, R)                                                                       \
    hipLaunchKernelGGL((sx::spmm_csr_rowgroup<LPR, CH, EX, ST, R>), dim3(nwg), dim3(sx::kBlock), 0, \
                       s, rp, rend, ci, va, dBp, pstride, dCin, ldc_in, dCout, ldc, row_begin,          \
                       row_end, ntiles, nrowblk, alpha, beta, xcd, skip, groups)
    // The LDS-staged A stream walks a block's non-zeros in order, which serialises row groups when rows
    // are long pieces of one hub row (split mode): there every row group streams its own piece directly.
    const bool stage = h->opt_stage && !pieces;
    if (rm_ldb > 0) {
        if (h->opt_exact) { if (stage) SX_LAUNCH(true, true, true); else SX_LAUNCH(true, false, true); }
        else              { if (stage) SX_LAUNCH(false, true, true); else SX_LAUNCH(false, false, true); }
        return;
    }
    if (h->opt_exact) { if (stage) SX_LAUNCH(true, true, false); else SX_LAUNCH(true, false, false); }
    else              { if (stage) SX_LAUNCH(false, true, false); else SX_LAUNCH(false, false, false); }
#undef SX_LAUNCH
}

// dBp: repacked panel (bcol_ld == 0) or the caller's column-major B at this segment's first column with its
// leading dimension bcol_ld (dictionary-only plans, small B: no repack launch).
template <int LPR>
int launch_panel(sextans_engine *h, const float *dBp, const float *dCin, int64_t ldc_in, float *dCout,
                  int64_t ldc, int ntiles, float alpha, float beta, hipStream_t s, int64_t bcol_ld, int blk_begin,
                  int blk_end, int row_base) {
    constexpr int RB = sx::kBlock / LPR;
    constexpr int NT = 4 * LPR;
    const int nblk = blk_end - blk_begin;
    if (nblk <= 0) return SEXTANS_OK;
    if (int rc = restore_plan_streams(h)) return rc;   // (released while a clustered plan served the whole-matrix calls)
    const unsigned nwg = (unsigned)nblk * (unsigned)ntiles;
    const int64_t pstride = bcol_ld > 0 ? bcol_ld : (int64_t)h->K * NT;
    const int xcd = (int)h->opt_xcd;
    // LDS = B panel sized for the largest dictionary of this matrix (rounded to 1 KiB) + C tile.
    const int pad_rows = h->ps.d_ioff ? sx::kWidePadRows : 1;   // (shared index lists may be shifted: their padding entries reach further)
    const int panel_floats = (h->ps.plan_pad_row + pad_rows) * NT;   // dictionary capacity + the +1.0f rows the padding entries address
    const int tile_floats = NT * (RB + 1);   // the C tile reuses the panel bytes
    const size_t lds = (size_t)(panel_floats > tile_floats ? panel_floats : tile_floats) * sizeof(int);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(nwg), dim3(sx::kBlock), lds, s, (const int2 *)h->ps.d_row_off, h->ps.d_lidx,
                           h->ps.d_pcol32, h->ps.d_pval, h->ps.d_blk_row, h->ps.d_dict_ptr, h->ps.d_dict, h->ps.plan_dict_stride, dBp,
                           pstride, dCin, ldc_in, dCout, ldc, ntiles, nblk, alpha, beta, xcd, panel_floats,
                           (long long *)h->d_dbg, blk_begin, row_base, (const unsigned char *)h->d_skip, (const int2 *)h->ps.d_ioff, pad_rows);
    };
    if (h->ps.plan_mixed) {
        if (h->opt_exact) go(sx::spmm_csr_panel<LPR, true, true>);
        else go(sx::spmm_csr_panel<LPR, false, true>);
    } else if (bcol_ld > 0) {
        if (h->opt_exact) go(sx::spmm_csr_panel<LPR, true, false, true>);
        else go(sx::spmm_csr_panel<LPR, false, false, true>);
    } else {
        if (h->opt_exact) go(sx::spmm_csr_panel<LPR, true, false>);
        else go(sx::spmm_csr_panel<LPR, false, false>);
    }
    return SEXTANS_OK;
}

// Wide-N form of the panel kernel (spmm_panel_v2.h): `nsuper` super tiles of 32 columns starting at the pointers
// given; dictionary-only plans built for 4 lanes per row.
// Workgroup placement of the reordered form at N <= 32: false = row blocks to the XCDs round-robin (round 4, commit ad33d1a), true =
// contiguous chunks like every other launch.  Re-decided in round 5 with fabric traffic as a criterion: DESIGN 9 / profiles/r05_xcd_placement_ab.txt.
constexpr bool kReorderedContiguous = true;
template <int H>
int launch_panel_v2(sextans_engine *h, const float *dBp, const float *dCin, int64_t ldc_in, float *dCout, int64_t ldc,
                      int nsuper, float alpha, float beta, hipStream_t s, int64_t bcol_ld, int blk_begin, int blk_end,
                      int row_base, int mode = 0, int last_cols = 16, int64_t rm_ldb = 0, bool dict_blocks_only = false) {
    // dict_blocks_only (mixed plan, split form): the launch walks P.d_dict_blocks instead of [blk_begin, blk_end)
    // rm_ldb > 0 (sextans_spmm_device_rm): dBp is the caller's ROW-major B with that leading dimension, dCin / dCout its row-major C
    // (ldc_in / ldc = row strides); mode 2 then reads B through the plan's dictionaries translated back to the caller's column
    // numbers (h->d_dict_nat) instead of permuted panels.
    // mode 1 (grid bricks): the plan over the rows in brick order, whole-matrix calls only; its slot -> row table addresses C.
    // mode 2 (graph clustering, the reordered form): dBp = permuted panels, dCin == dCout == the row-major staging buffer,
    // ldc_in == ldc == floats per tile; the same slot -> row table addresses the staging rows.
    // mode 3 (clustered-order chunks of sextans_dist_spmm): the graph-clustered plan with C addressed BY POSITION in the clustered order
    // (no slot -> row table): dCin == dCout == a packed slab [tile][position][16] of the chunk, ldc_in == ldc == floats per tile.
    const sextans_engine::PanelState &P = mode ? h->psc : h->ps;
    const int *slot_row = (mode == 1 || mode == 2) ? h->d_slot_row : nullptr;
    const unsigned char *skip = mode == 3 ? nullptr : (const unsigned char *)h->d_skip;   // rows on the piece path: never written by this kernel (mode 2: their staging rows keep C_in)
    const bool crow = mode == 2 || mode == 3;
    const int nblk = dict_blocks_only ? P.n_dict_blocks : blk_end - blk_begin;
    if (nblk <= 0 || nsuper <= 0) return SEXTANS_OK;
    if (mode == 0)
        if (int rc = restore_plan_streams(h)) return rc;   // (released while a clustered plan served the whole-matrix calls)
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
    const bool big = H == 1 && bcol_ld > 0 && nb > 2;   // column-major staging + long rows: the 256-register form (2 workgroups per CU)
    int tpw = (int)h->opt_tiles_per_wg;
    if (tpw <= 0 && big) {   // ... in ONE round of workgroups
        tpw = std::min<int>(nsuper, std::max<int>(1, (int)(((int64_t)nblk * nsuper + 2 * h->num_cus - 1) / ((int64_t)2 * h->num_cus))));
    } else if (tpw <= 0 && rm_ldb > 0 && P.plan_sets == 2 && nsuper >= 4) {
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
    tpw = std::min(tpw, nsuper);
    const int ngrp = (nsuper + tpw - 1) / tpw;
    const bool rm = rm_ldb > 0;
    const int64_t pstride = rm ? rm_ldb : bcol_ld > 0 ? bcol_ld : (int64_t)h->K * 16;
    const int *dict = (rm && crow && h->d_dict_nat) ? h->d_dict_nat : P.d_dict;
    // LDS = the panel: plan capacity + the +1.0f row.  A clustered plan of a short-row matrix is packed for a 320-row panel
    // (engine_plan.hip: small_panel): 20.5 KB instead of 36.9 KB per workgroup, so the CU holds as many workgroups as the registers
    // allow (5 at <= 96 registers) instead of the 4 the full panel permits -- these launches are latency-bound
    const bool small_panel = H == 1 && bcol_ld == 0 && P.plan_pad_row == 5 * 64;
    const size_t lds = small_panel ? (size_t)(5 * 64 + sx::kWidePadRows) * 64 : (size_t)H * sx::kWideHalfBytes;
    // contiguous chunks of row blocks per XCD -- except the reordered form at N <= 32, where handing the blocks of the merge-tree order to
    // the XCDs round-robin measured 1.3 .. 4.5 % faster (renumbered FEM 607 -> 582 us, unstructured mesh 444 -> 424; N = 128: +1.4 % the other way)
    // ("reordered_xcd": measurement switch for exactly this decision -- 0 round-robin, 1 contiguous chunks, -1 the rule above)
    const int xcd = crow && h->opt_reordered_xcd >= 0 ? (int)h->opt_reordered_xcd : (crow && nsuper <= 2 && !kReorderedContiguous) ? 0 : (int)h->opt_xcd;
    auto go = [&](auto kern) -> int {
        if (int rc = allow_big_lds(h, reinterpret_cast<const void *>(kern), (int)lds)) return rc;
        hipLaunchKernelGGL(kern, dim3((unsigned)nblk * (unsigned)ngrp), dim3(sx::kBlock), lds, s, (const int2 *)P.d_row_off,
                           P.d_lidx, P.d_pval, P.d_blk_row, P.d_dict_ptr, dict, P.plan_dict_stride,
                           dBp, pstride, dCin, ldc_in, dCout, ldc, nsuper, tpw, nblk, alpha, beta, xcd,
                           P.plan_pad_row, blk_begin, row_base, skip, (long long *)h->d_dbg, slot_row, (const int2 *)P.d_ioff, last_cols, dict_blocks_only ? (const int *)P.d_dict_blocks : (const int *)nullptr);
        return SEXTANS_OK;
    };
    if constexpr (H > 1) {
        if (bcol_ld > 0) return h->opt_exact ? go(sx::spmm_csr_panel_v2<H, 6, true, true>) : go(sx::spmm_csr_panel_v2<H, 6, false, true>);
        return h->opt_exact ? go(sx::spmm_csr_panel_v2<H, 6, true, false>) : go(sx::spmm_csr_panel_v2<H, 6, false, false>);
    } else {
        // small matrices staged from column-major B: dictionary capacity from the plan (5 x 64 covers nasa4704's 300)
        const bool small_dict = bcol_ld > 0 && P.plan_max_dict <= 5 * 64;
        if (h->opt_phase_timing && h->d_dbg && h->opt_exact && P.plan_sets == 1) {   // diagnostic instantiations: the forms the dispatcher uses most
            if (small_dict && nb == 3 && h->opt_small_v2 != 0) return go(sx::spmm_csr_panel_v2<H, 3, true, true, true, 5>);
            if (bcol_ld > 0) return go(sx::spmm_csr_panel_v2<H, 2, true, true, true>);
            if (nb == 6 && !crow && !small_panel) return go(sx::spmm_csr_panel_v2<H, 6, true, false, true>);
            if (nb == 2 && !crow && small_panel) return go(sx::spmm_csr_panel_v2<H, 2, true, false, true, 5>);
        }
        if (small_dict && h->opt_small_v2 != 0) {
            if (nb == 3) return h->opt_exact ? go(sx::spmm_csr_panel_v2<H, 3, true, true, false, 5>) : go(sx::spmm_csr_panel_v2<H, 3, false, true, false, 5>);
            return h->opt_exact ? go(sx::spmm_csr_panel_v2<H, 2, true, true, false, 5>) : go(sx::spmm_csr_panel_v2<H, 2, false, true, false, 5>);
        }
        if (big) {
            if (nb <= 4) return h->opt_exact ? go(sx::spmm_csr_panel_v2<H, 4, true, true, false, 9, false, true>) : go(sx::spmm_csr_panel_v2<H, 4, false, true, false, 9, false, true>);
            return h->opt_exact ? go(sx::spmm_csr_panel_v2<H, 6, true, true, false, 9, false, true>) : go(sx::spmm_csr_panel_v2<H, 6, false, true, false, 9, false, true>);
        }
        if (bcol_ld > 0) return h->opt_exact ? go(sx::spmm_csr_panel_v2<H, 2, true, true>) : go(sx::spmm_csr_panel_v2<H, 2, false, true>);
        if (rm) {   // the caller's row-major operands: the 16-byte C accesses of the staging form on the caller's own rows, B without a repack
// (C beyond 4 GB -- M * ldc * 4 bytes -- takes the instantiations with 64-bit lane addresses: RM == 2)
            const bool c64 = (int64_t)h->M * std::max(ldc, ldc_in) * 4 >= ((int64_t)1 << 32);
#define SX_RM1(NBV, DC, ST, R) (h->opt_exact ? go(sx::spmm_csr_panel_v2<H, NBV, true, false, false, DC, true, false, ST, R>) \
                                             : go(sx::spmm_csr_panel_v2<H, NBV, false, false, false, DC, true, false, ST, R>))
#define SX_RM(NBV, DC, ST) (c64 ? SX_RM1(NBV, DC, ST, 2) : SX_RM1(NBV, DC, ST, 1))
            if (P.plan_sets == 2) return SX_RM(2, 9, 2);
            if (small_panel) return nb >= 3 ? SX_RM(3, 5, 1) : SX_RM(2, 5, 1);
            if (nb == 3) return SX_RM(3, 9, 1);
            if (nb == 2) return SX_RM(2, 9, 1);
            if (nb == 4) return SX_RM(4, 9, 1);
            return SX_RM(6, 9, 1);
#undef SX_RM1
#undef SX_RM
        }
        if (P.plan_sets == 2) {   // two row sets per block (short-row clustered plans: every row has <= 32 entries = 2 register-resident batches)
            if (crow) return h->opt_exact ? go(sx::spmm_csr_panel_v2<H, 2, true, false, false, 9, true, false, 2>) : go(sx::spmm_csr_panel_v2<H, 2, false, false, false, 9, true, false, 2>);
            return h->opt_exact ? go(sx::spmm_csr_panel_v2<H, 2, true, false, false, 9, false, false, 2>) : go(sx::spmm_csr_panel_v2<H, 2, false, false, false, 9, false, false, 2>);
        }
        if (small_panel && crow) {
            if (nb >= 3) return h->opt_exact ? go(sx::spmm_csr_panel_v2<H, 3, true, false, false, 5, true>) : go(sx::spmm_csr_panel_v2<H, 3, false, false, false, 5, true>);
            return h->opt_exact ? go(sx::spmm_csr_panel_v2<H, 2, true, false, false, 5, true>) : go(sx::spmm_csr_panel_v2<H, 2, false, false, false, 5, true>);
        }
        if (small_panel) {
            if (nb >= 3) return h->opt_exact ? go(sx::spmm_csr_panel_v2<H, 3, true, false, false, 5>) : go(sx::spmm_csr_panel_v2<H, 3, false, false, false, 5>);
            return h->opt_exact ? go(sx::spmm_csr_panel_v2<H, 2, true, false, false, 5>) : go(sx::spmm_csr_panel_v2<H, 2, false, false, false, 5>);
        }
        if (crow) {   // block-major C staging
            if (nb == 3) return h->opt_exact ? go(sx::spmm_csr_panel_v2<H, 3, true, false, false, 9, true>) : go(sx::spmm_csr_panel_v2<H, 3, false, false, false, 9, true>);
            if (nb == 2) return h->opt_exact ? go(sx::spmm_csr_panel_v2<H, 2, true, false, false, 9, true>) : go(sx::spmm_csr_panel_v2<H, 2, false, false, false, 9, true>);
            if (nb == 4) return h->opt_exact ? go(sx::spmm_csr_panel_v2<H, 4, true, false, false, 9, true>) : go(sx::spmm_csr_panel_v2<H, 4, false, false, false, 9, true>);
            return h->opt_exact ? go(sx::spmm_csr_panel_v2<H, 6, true, false, false, 9, true>) : go(sx::spmm_csr_panel_v2<H, 6, false, false, false, 9, true>);
        }
        if (nb == 3) return h->opt_exact ? go(sx::spmm_csr_panel_v2<H, 3, true, false>) : go(sx::spmm_csr_panel_v2<H, 3, false, false>);
        if (nb == 2) return h->opt_exact ? go(sx::spmm_csr_panel_v2<H, 2, true, false>) : go(sx::spmm_csr_panel_v2<H, 2, false, false>);
        if (nb == 4) return h->opt_exact ? go(sx::spmm_csr_panel_v2<H, 4, true, false>) : go(sx::spmm_csr_panel_v2<H, 4, false, false>);
        return h->opt_exact ? go(sx::spmm_csr_panel_v2<H, 6, true, false>) : go(sx::spmm_csr_panel_v2<H, 6, false, false>);
    }
}

// dBp8: N/8 row-major K x 8 panels.  Rows [wave_begin * RW, min(M, wave_end * RW)); the C pointers address
// row `row_base` as their row 0.
void launch_window(sextans_engine *h, const float *dBp8, const float *dCin, int64_t ldc_in, float *dCout,
                   int64_t ldc, int ntiles, int wave_begin, int wave_end, int row_base, float alpha, float beta,
                   hipStream_t s) {
    const int nwg = (wave_end - wave_begin + sx::kWinWaves - 1) / sx::kWinWaves;
    if (nwg <= 0) return;
    const size_t lds = (size_t)sx::kWinWaves * (size_t)(h->win_rw + 1) * sx::kWinNT * sizeof(float);
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)nwg * (unsigned)ntiles), dim3(sx::kWinWaves * 64), lds, s,
                           (const sx::u32x2 *)h->d_wstream, (const int *)h->d_wstep0, dBp8, (int64_t)h->K * sx::kWinNT, dCin,
                           ldc_in, dCout, ldc, h->M, h->win_rw, wave_begin, wave_end, nwg, row_base, alpha, beta,
                           (const unsigned char *)h->d_skip);
    };
    if (h->opt_win_unroll == 4) { if (h->opt_exact) go(sx::spmm_csr_window<true, 4>); else go(sx::spmm_csr_window<false, 4>); }
    else                        { if (h->opt_exact) go(sx::spmm_csr_window<true, 8>); else go(sx::spmm_csr_window<false, 8>); }
}

// ---- clustered-order chunks of the row-partitioned SpMM (engine_dist.hip: sextans_dist_spmm with nchunks > 1) -------------------
// A rank whose slab runs on a graph-clustered plan used to lose it as soon as the slab was cut into chunks for the all-gather
// pipeline: a row-range call needs consecutive rows, and the clustered plan has none.  Here a chunk is a range of the plan's ROW
// BLOCKS; its rows are the positions [p0, p1) of the clustered order, and everything the chunk moves is addressed by position:
//   cc_pre      (first chunk) B into the permuted panels, the slab of C_in into the natural row-major staging buffer (streaming passes);
//   cc_chunk    C_in rows of the chunk gathered, 64 bytes each, into the chunk's packed slab [tile][position][16] -- which IS the
//               rank's slot of the all-gather buffer -- then spmm_csr_panel_v2<..., CROW> over the chunk's blocks, in place;
//   cc_scatter  (every rank, behind the all-gather) rows of a received slab to their places in a row-major staging buffer of the
//               WHOLE C through the sender's position -> row table;
//   cc_finish   one streaming pass staging -> column-major C.
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
__global__ __launch_bounds__(256) void position_rows(int nblk, int RB, const int *__restrict__ blk_row, const int *__restrict__ slot_row, int row0, int *__restrict__ out) {
    const int b = blockIdx.x, s = threadIdx.x;
    if (b >= nblk || s >= RB) return;
    const int p0 = blk_row[b], n = blk_row[b + 1] - p0;
    if (s < n) out[p0 + s] = slot_row[(int64_t)b * RB + s] + row0;
}
}  // namespace

bool cc_usable(sextans_engine *h, int N, const Tiling &t) {
    return h->cluster_state == 2 && h->cluster_cm_pays && t.W == 16 && N % 16 == 0 && t.segs.size() == 1 && t.segs[0].width == 16 && h->nhub == 0 &&
           h->nchain == 0 && csr_only(h) && (h->opt_kernel == 0 || h->opt_kernel == 2) && h->d_Cs && h->d_slot_row &&
           h->Cs_cap >= (size_t)(N / 16) * (size_t)h->M * 16 && h->Bp_cap >= (size_t)h->K * (size_t)N && h->psc.plan_sets == 1 &&
           (h->M >= 65536 || h->m_nnz * (int64_t)N >= ((int64_t)24 << 20)) && (int)h->psc.h_blk_row.size() == h->psc.plan_nblk + 1;
}
void cc_table(sextans_engine *h, int row0, int *d_out, hipStream_t s) {
    const int slots = sx::kBlock / 4 * std::max(1, h->psc.plan_sets);   // (grid-brick plans of short-row matrices: two row sets per block)
    hipLaunchKernelGGL(position_rows, dim3((unsigned)h->psc.plan_nblk), dim3((unsigned)slots), 0, s, h->psc.plan_nblk, slots, h->psc.d_blk_row, h->d_slot_row, row0, d_out);
}
void cc_pre(sextans_engine *h, int N, const float *d_B, int64_t ldb, const float *d_C_in_slab, int64_t ldc_in, hipStream_t s) {
    Prof p(h, &h->ev_repack, s);
    if (h->d_colpos)
        hipLaunchKernelGGL(sx::repack_b_panels_perm, dim3((unsigned)((h->col_hi - h->col_lo + sx::kBlock - 1) / sx::kBlock), (unsigned)(N / 16)), dim3(sx::kBlock), 0, s,
                           d_B, ldb, h->d_Bp, h->K, 0, h->d_colpos, h->col_lo, h->col_hi, N, h->d_touched);
    else
        launch_repack<16>(d_B, ldb, h->d_Bp, h->K, 0, N / 16, s, h->col_lo, h->col_hi, -1, h->d_touched);
    launch_repack<16>(d_C_in_slab, ldc_in, h->d_Cs, h->M, 0, N / 16, s);
    h->bp_layout = -16;
}
int cc_chunk(sextans_engine *h, int N, float alpha, float beta, int b0, int b1, const int *d_rows, int row0, float *slab, int64_t lmax, hipStream_t s) {
    const int p0 = h->psc.h_blk_row[(size_t)b0], p1 = h->psc.h_blk_row[(size_t)b1];
    if (p1 <= p0) return SEXTANS_OK;
    Prof p(h, &h->ev_kernel, s);
    hipLaunchKernelGGL(slab_rows<false>, dim3((unsigned)(((int64_t)(p1 - p0) * 4 + 255) / 256), (unsigned)(N / 16)), dim3(256), 0, s, h->d_Cs, (int64_t)h->M * 16,
                       d_rows + p0, row0, p1 - p0, slab, lmax * 16);
    float *base = slab - (int64_t)p0 * 16;     // position p of the clustered order -> slab row p - p0
    if (int rc = launch_panel_v2<1>(h, h->d_Bp, base, lmax * 16, base, lmax * 16, N / 16, alpha, beta, s, 0, b0, b1, 0, 3)) return rc;
    h->last_kernel = "spmm_csr_panel_v2_reordered";
    return SEXTANS_OK;
}
void cc_scatter(const float *slab, int64_t lmax, const int *d_rows, int n, float *tiles, int64_t tile_stride, int N, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(slab_rows<true>, dim3((unsigned)(((int64_t)n * 4 + 255) / 256), (unsigned)(N / 16)), dim3(256), 0, s, tiles, tile_stride, d_rows, 0, n,
                       const_cast<float *>(slab), lmax * 16);
}
void cc_finish(const float *tiles, float *C, int64_t ldc, int M_total, int N, hipStream_t s) {
    hipLaunchKernelGGL(sx::tiles_to_colmajor, dim3((unsigned)((M_total + sx::kBlock - 1) / sx::kBlock), (unsigned)(N / 16)), dim3(sx::kBlock), 0, s, tiles, C, ldc,
                       M_total, 0, N);
}
int cc_prepare(sextans_engine *h, int N, bool *ok) {
    Tiling t;
    *ok = false;
    if (int rc = prepare(h, N, true, &t)) return rc;
    *ok = cc_usable(h, N, t);
    return SEXTANS_OK;
}

static const struct { const char *key; int64_t sextans_engine::*slot; } kOptions[] = {
    {"kernel", &sextans_engine::opt_kernel}, {"lanes_per_row", &sextans_engine::opt_lpr}, {"stage_a", &sextans_engine::opt_stage},
    {"xcd_remap", &sextans_engine::opt_xcd}, {"exact", &sextans_engine::opt_exact}, {"profile", &sextans_engine::opt_profile},
    {"panel_min_reuse_x100", &sextans_engine::opt_min_reuse_x100}, {"panel_min_reuse_wide_x100", &sextans_engine::opt_min_reuse_wide_x100},
    {"phase_timing", &sextans_engine::opt_phase_timing}, {"split_rows", &sextans_engine::opt_split_rows},
    {"bucket_rows", &sextans_engine::opt_bucket_rows}, {"global_nnz", &sextans_engine::opt_global_nnz},
    {"exact_chain", &sextans_engine::opt_exact_chain}, {"fuse_b", &sextans_engine::opt_fuse_b}, {"cols_per_lane", &sextans_engine::opt_cols_per_lane},
    {"tiles_per_wg", &sextans_engine::opt_tiles_per_wg}, {"panel_v2", &sextans_engine::opt_panel_v2}, {"small_v2", &sextans_engine::opt_small_v2},
    {"row_cluster", &sextans_engine::opt_row_cluster}, {"cluster_top", &sextans_engine::opt_cluster_top}, {"small_panel", &sextans_engine::opt_small_panel}, {"row_sets", &sextans_engine::opt_row_sets},
    {"row_offset", &sextans_engine::opt_row_offset}, {"relabel_columns", &sextans_engine::opt_relabel_columns},
    {"row_similarity", &sextans_engine::opt_row_similarity}, {"reordered_xcd", &sextans_engine::opt_reordered_xcd},
    {"run_cluster", &sextans_engine::opt_run_cluster}, {"refine_sweeps", &sextans_engine::opt_refine_sweeps},
    {"share_index", &sextans_engine::opt_share_index}, {"refine_rows", &sextans_engine::opt_refine_rows},
    {"colwise_max_len", &sextans_engine::opt_colwise_max_len}, {"colwise_tiles_adjacent", &sextans_engine::opt_colwise_tiles_adjacent},
    {"split_mixed", &sextans_engine::opt_split_mixed}, {"cluster_shape", &sextans_engine::opt_cluster_shape},
    {"cluster_group", &sextans_engine::opt_cluster_group}, {"window_rows", &sextans_engine::opt_win_rows},
    {"window_cols", &sextans_engine::opt_win_cols}, {"window_unroll", &sextans_engine::opt_win_unroll},
    {"window_auto", &sextans_engine::opt_win_auto}, {"bell_wide", &sextans_engine::opt_bell_wide}, {"bell_generation", &sextans_engine::opt_bell_gen},
    {"bell_shared", &sextans_engine::opt_bell_shared}, {"bell_debug", &sextans_engine::opt_bell_debug},
    {"dist_broadcast_runs", &sextans_engine::opt_dist_broadcast_runs}, {"rowblock_tiles", &sextans_engine::opt_rb_tiles},
    {"mfma_dense_tiles", &sextans_engine::opt_mfma_dense}, {"dense_tile_fill_x100", &sextans_engine::opt_dense_fill_x100},
};

// The transposed form carries the options of its engine (sextans_spmm_t_device_rm) -- except "row_offset" and "global_nnz", which
// describe a row slab of the multi-GPU forms, not A^T.  key == nullptr: all of them (the companion was just created).
int transposed_options(sextans_engine *h, const char *key, int64_t value) {
    auto skip = [](const char *k) { return !strcmp(k, "row_offset") || !strcmp(k, "global_nnz"); };
    if (key) return skip(key) ? SEXTANS_OK : sextans_set_option(h->tr, key, value);
    for (const auto &o : kOptions)
        if (!skip(o.key) && h->tr->*o.slot != h->*o.slot)
            if (int rc = sextans_set_option(h->tr, o.key, h->*o.slot)) return rc;
    h->tr->opt_mode = h->opt_mode;
    return SEXTANS_OK;
}

}  // namespace sxe

extern "C" {

const char *sextans_last_error(void) { return g_last_error.c_str(); }

int sextans_device_count(int *count) {
    if (!count) return SEXTANS_ERR_INVALID;
    *count = 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return SEXTANS_ERR_NO_DEVICE;
    int ok = 0;
    for (int d = 0; d < n; ++d)
        if (check_device(d) == SEXTANS_OK) ++ok;
    *count = ok;
    return ok > 0 ? SEXTANS_OK : SEXTANS_ERR_NO_DEVICE;
}

int sextans_create(sextans_handle_t *out, int device) {
    if (!out) return SEXTANS_ERR_INVALID;
    *out = nullptr;
    if (int rc = check_device(device)) return rc;
    SX_HIP(hipSetDevice(device));
    auto *h = new sextans_engine();
    h->device = device;
    {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, device) == hipSuccess && p.multiProcessorCount > 0)
            h->num_cus = p.multiProcessorCount;
    }
    {   // load the device code now (the runtime does it lazily at the first launch, ~1 ms, which would
        // otherwise land inside the first timed SpMM)
        hipFuncAttributes fa;
        (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(&sx::repack_b_panels<16>));
        (void)hipGetLastError();
    }
    *out = h;
    return SEXTANS_OK;
}

int sextans_destroy(sextans_handle_t h) {
    if (!h) return SEXTANS_ERR_INVALID;
    (void)hipSetDevice(h->device);
    free_matrix(h);
    free_bell(h);
    (void)hipFree(h->d_bell_Bf);
    (void)hipFree(h->d_Bp); (void)hipFree(h->d_B); (void)hipFree(h->d_Cin); (void)hipFree(h->d_Cout); (void)hipFree(h->d_Cs);
    sextans_profile_reset(h);
    (void)hipFree(h->d_P);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    if (h->aux_stream) (void)hipStreamDestroy(h->aux_stream);
    (void)hipFree(h->d_dbg);
    (void)hipFree(h->d_chB); (void)hipFree(h->d_chC);
    (void)hipFree(h->d_stage);
    (void)hipFree(h->d_Cfull); (void)hipFree(h->d_dist_rows); (void)hipFree(h->d_rmB); (void)hipFree(h->d_rmC);
    for (hipEvent_t e : h->dist_events) (void)hipEventDestroy(e);
    if (h->comm_stream) (void)hipStreamDestroy(h->comm_stream);
    if (h->host_stream) (void)hipStreamDestroy(h->host_stream);
    delete h;
    return SEXTANS_OK;
}

static int64_t *option_slot(sextans_handle_t h, const char *key) {
    for (const auto &o : kOptions)
        if (!strcmp(key, o.key)) return &(h->*o.slot);
    return nullptr;
}

int sextans_set_option(sextans_handle_t h, const char *key, int64_t value) {
    if (!h || !key) return SEXTANS_ERR_INVALID;
    if (!strcmp(key, "mode")) {   // the documented pair of accuracy modes (include/sextans_amd.h): one switch instead of three options nobody finds
        if (value != SEXTANS_MODE_STRICT && value != SEXTANS_MODE_FAST) return SEXTANS_ERR_INVALID;
        const bool fast = value == SEXTANS_MODE_FAST;
        if (int rc = sextans_set_option(h, "exact", fast ? 0 : 1)) return rc;
        if (int rc = sextans_set_option(h, "split_rows", fast ? -1 : 0)) return rc;
        // ("mfma_dense_tiles" = 2 -- dense row blocks on the fp32 matrix cores -- never changes a bit against "exact" = 0, but as measured in
        // round 6 it does not beat the VALU kernels either (profiles/r06_rowblock_mfma.jsonl): it stays an option of its own, off in both modes)
        if (int rc = sextans_set_option(h, "mfma_dense_tiles", 0)) return rc;
        h->opt_mode = value;
        if (h->tr) h->tr->opt_mode = value;
        return SEXTANS_OK;
    }
    int64_t *slot = option_slot(h, key);
    if (!slot) return SEXTANS_ERR_INVALID;
    // Measurement switches -- ablation bits that corrupt C on purpose ("bell_debug"), brick shapes and groupings of the clustered
    // row order, per-phase cycle counters -- are not part of the drop-in surface: they exist only for processes started with
    // SEXTANS_DEBUG_OPTIONS=1 (tools/), and a value other than the default is refused otherwise.
    if (slot == &h->opt_bell_debug || slot == &h->opt_cluster_shape || slot == &h->opt_cluster_group || slot == &h->opt_phase_timing || slot == &h->opt_reordered_xcd ||
        slot == &h->opt_dist_broadcast_runs || slot == &h->opt_rb_tiles) {
        const char *dbg = getenv("SEXTANS_DEBUG_OPTIONS");
        if (!(dbg && dbg[0] == '1') && value != *slot) {
            g_last_error = std::string("option \"") + key + "\" is a measurement switch: set SEXTANS_DEBUG_OPTIONS=1 in the environment to use it";
            return SEXTANS_ERR_INVALID;
        }
    }
    if (slot == &h->opt_cluster_shape && value != 0) {   // run_rows * 10000 + lines * 100 + planes, every factor >= 1, <= 4096 rows per brick
        const int64_t rr = value / 10000, b2 = value / 100 % 100, b3 = value % 100;
        if (value < 0 || rr < 1 || b2 < 1 || b3 < 1 || rr * b2 * b3 > 4096) return SEXTANS_ERR_INVALID;
    }
    if (slot == &h->opt_cluster_group && (value < 1 || value > 64)) return SEXTANS_ERR_INVALID;
    if (slot == &h->opt_panel_v2 && (value < -1 || value > 1)) return SEXTANS_ERR_INVALID;
    if (slot == &h->opt_row_cluster && (value < -1 || value > 2)) return SEXTANS_ERR_INVALID;
    if (slot == &h->opt_row_similarity && (value < -1 || value > 1)) return SEXTANS_ERR_INVALID;
    if (slot == &h->opt_lpr && value != 0 && value != 2 && value != 4 && value != 8) return SEXTANS_ERR_INVALID;
    if (slot == &h->opt_win_rows && (value < 1 || value > sx::kWinMaxRowsPerWave)) return SEXTANS_ERR_INVALID;
    if (slot == &h->opt_win_cols && (value < 1 || value > 0x7fffffff)) return SEXTANS_ERR_INVALID;
    if (slot == &h->opt_win_unroll && value != 4 && value != 8) return SEXTANS_ERR_INVALID;
    if (slot == &h->opt_cols_per_lane && value != 0 && value != 4 && value != 8) return SEXTANS_ERR_INVALID;
    if (slot == &h->opt_tiles_per_wg && (value < 0 || value > 1024)) return SEXTANS_ERR_INVALID;
    if ((slot == &h->opt_win_rows || slot == &h->opt_win_cols) && *slot != value) {
        (void)hipSetDevice(h->device);
        free_window(h);   // the stream is built for one (rows per wavefront, window) pair
    }
    if ((slot == &h->opt_row_cluster || slot == &h->opt_cluster_top || slot == &h->opt_small_panel || slot == &h->opt_row_sets || slot == &h->opt_row_offset || slot == &h->opt_relabel_columns || slot == &h->opt_row_similarity || slot == &h->opt_run_cluster || slot == &h->opt_refine_sweeps || slot == &h->opt_refine_rows || slot == &h->opt_cluster_shape || slot == &h->opt_cluster_group || slot == &h->opt_min_reuse_x100 || slot == &h->opt_min_reuse_wide_x100) && *slot != value) {
        (void)hipSetDevice(h->device);   // the clustered-order plan is (re)considered under the new setting
        free_cluster_plan(h);
        h->cluster_rm_tried = false;
    }
    if (slot == &h->opt_colwise_max_len && *slot != value) h->colwise_state = 0;
    // (every packed form is rebuilt; "split_mixed" moves the share of blocks with reuse from which a mixed plan is built at all, and a
    // cached "not built" verdict or a plan built under the other threshold must not survive the toggle)
    if ((slot == &h->opt_share_index || slot == &h->opt_split_mixed) && *slot != value) { (void)hipSetDevice(h->device); free_plan(h); }
    if (*slot != value) h->dist_cut_key.clear();   // chunk cuts are aligned to the packed forms the options select (all
                                                   // ranks of a partition must change options together: the cut
                                                   // exchange is a collective)
    *slot = value;
    if (slot == &h->opt_phase_timing) {
        (void)hipSetDevice(h->device);
        if (value && !h->d_dbg && hipMalloc((void **)&h->d_dbg, 64) != hipSuccess) return SEXTANS_ERR_HIP;
        if (h->d_dbg) (void)hipMemset(h->d_dbg, 0, 64);
        if (!value && h->d_dbg) { (void)hipFree(h->d_dbg); h->d_dbg = nullptr; }
    }
    return h->tr ? transposed_options(h, key, value) : SEXTANS_OK;
}

int sextans_phase_timing_read(sextans_handle_t h, int64_t out[8]) {
    if (!h || !out || !h->d_dbg) return SEXTANS_ERR_STATE;
    SX_HIP(hipSetDevice(h->device));
    SX_HIP((hipDeviceSynchronize)());   // (debug aid: the kernels that wrote d_dbg ran on the caller's streams)
    SX_HIP(hipMemcpy(out, h->d_dbg, 64, hipMemcpyDeviceToHost));
    return SEXTANS_OK;
}

int sextans_get_option(sextans_handle_t h, const char *key, int64_t *value) {
    if (!h || !key || !value) return SEXTANS_ERR_INVALID;
    if (!strcmp(key, "mode")) {   // what the three options it stands for say now (-1: set apart by hand)
        const bool strict = h->opt_exact == 1 && h->opt_split_rows == 0 && h->opt_mfma_dense == 0;
        const bool fast = h->opt_exact == 0 && h->opt_split_rows == -1 && h->opt_mfma_dense == 0;
        *value = strict ? SEXTANS_MODE_STRICT : fast ? SEXTANS_MODE_FAST : -1;
        return SEXTANS_OK;
    }
    int64_t *slot = option_slot(h, key);
    if (!slot) return SEXTANS_ERR_INVALID;
    *value = *slot;
    return SEXTANS_OK;
}

int sextans_set_matrix_csr(sextans_handle_t h, int M, int K, int64_t nnz, const int *row_ptr,
                           const int *col_idx, const float *val) {
    if (!h || M < 0 || K < 0 || nnz < 0 || !row_ptr || (nnz > 0 && (!col_idx || !val)))
        return SEXTANS_ERR_INVALID;
    if (nnz > 0x7fffffffLL) return SEXTANS_ERR_INVALID;   // 32-bit row_ptr like the reference
    if (row_ptr[0] != 0 || row_ptr[M] != (int)nnz) return SEXTANS_ERR_INVALID;
    // the kernels gather B rows by column index and the plan builders index host arrays of size K with them
    for (int r = 0; r < M; ++r)
        if (row_ptr[r + 1] < row_ptr[r]) return SEXTANS_ERR_INVALID;
    {
        unsigned bad = 0;
        for (int64_t j = 0; j < nnz; ++j) bad |= (unsigned)((unsigned)col_idx[j] >= (unsigned)K);
        if (bad) return SEXTANS_ERR_INDEX;
    }
    SX_HIP(hipSetDevice(h->device));
    free_matrix(h);
    int *rp = nullptr, *ci = nullptr;
    float *v = nullptr;
    SX_HIP(hipMalloc((void **)&rp, sizeof(int) * ((size_t)M + 1)));
    SX_HIP(hipMalloc((void **)&ci, sizeof(int) * (size_t)(nnz ? nnz : 1)));
    SX_HIP(hipMalloc((void **)&v, sizeof(float) * (size_t)(nnz ? nnz : 1)));
    SX_HIP(hipMemcpy(rp, row_ptr, sizeof(int) * ((size_t)M + 1), hipMemcpyHostToDevice));
    if (nnz) {
        SX_HIP(hipMemcpy(ci, col_idx, sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice));
        SX_HIP(hipMemcpy(v, val, sizeof(float) * (size_t)nnz, hipMemcpyHostToDevice));
    }
    h->d_rp = rp; h->d_ci = ci; h->d_v = v;
    h->owns_matrix = true;
    h->M = M; h->K = K; h->nnz = nnz;
    free_dense(h);   // source = main = the matrix itself until the dense-tile and long-row tests have run
    return SEXTANS_OK;
}

int sextans_set_matrix_csr_device(sextans_handle_t h, int M, int K, int64_t nnz,
                                  const int *d_row_ptr, const int *d_col_idx, const float *d_val) {
    if (!h || M < 0 || K < 0 || nnz < 0 || !d_row_ptr) return SEXTANS_ERR_INVALID;
    if (nnz > 0x7fffffffLL) return SEXTANS_ERR_INVALID;
    SX_HIP(hipSetDevice(h->device));
    free_matrix(h);
    h->d_rp = d_row_ptr; h->d_ci = d_col_idx; h->d_v = d_val;
    h->owns_matrix = false;
    h->M = M; h->K = K; h->nnz = nnz;
    free_dense(h);
    return SEXTANS_OK;
}

int sextans_spmm_device(sextans_handle_t h, int N, float alpha, const float *d_B, int64_t ldb,
                        float beta, const float *d_C_in, float *d_C_out, int64_t ldc,
                        void *stream) {
    return sextans_spmm_device2(h, N, alpha, d_B, ldb, beta, d_C_in, ldc, d_C_out, ldc, stream);
}

int sextans_align_row(sextans_handle_t h, int N, int row, int *aligned) {
    if (!h || !aligned || N <= 0 || (N % 8) != 0 || row < 0 || row > h->M) return SEXTANS_ERR_INVALID;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    SX_HIP(hipSetDevice(h->device));
    Tiling t;
    if (int rc = prepare(h, N, false, &t)) return rc;
    *aligned = row;
    if (row == h->M) return SEXTANS_OK;
    if (t.window) *aligned = row / h->win_rw * h->win_rw;
    else if (t.panel && !h->ps.h_blk_row.empty())
        *aligned = *(std::upper_bound(h->ps.h_blk_row.begin(), h->ps.h_blk_row.end(), row) - 1);
    return SEXTANS_OK;
}

int sextans_spmm_device2(sextans_handle_t h, int N, float alpha, const float *d_B, int64_t ldb,
                         float beta, const float *d_C_in, int64_t ldc_in, float *d_C_out, int64_t ldc,
                         void *stream) {
    if (!h) return SEXTANS_ERR_INVALID;
    return sextans_spmm_device_rows(h, N, alpha, d_B, ldb, beta, d_C_in, ldc_in, d_C_out, ldc, 0, h->M, 0,
                                    stream);
}

}  // extern "C"
namespace {
// Hub rows inside [row_begin, row_end): pieces summed as virtual rows by the row-group kernel from B panels of width
// 4 * LPR at dBp (ntiles panels), then folded in order into the C the main kernel has already written.
const char *with_rowblocks(sextans_engine *h, const char *name) {   // (sextans_last_kernel: the launches of this call + the fp32 matrix-core one)
    h->last_kernel_buf = std::string(name) + "+rowblock_mfma_f32";
    return h->last_kernel_buf.c_str();
}
const char *kernel_name(int main, bool hubs, bool dense) {   // static strings for sextans_last_kernel
    static const char *names[4][2][2] = {
        {{"spmm_csr_rowgroup", "spmm_csr_rowgroup+dense_tiles_mfma"},
         {"spmm_csr_rowgroup+hub_pieces", "spmm_csr_rowgroup+hub_pieces+dense_tiles_mfma"}},
        {{"spmm_csr_panel", "spmm_csr_panel+dense_tiles_mfma"},
         {"spmm_csr_panel+hub_pieces", "spmm_csr_panel+hub_pieces+dense_tiles_mfma"}},
        {{"spmm_csr_window", "spmm_csr_window+dense_tiles_mfma"},
         {"spmm_csr_window+hub_pieces", "spmm_csr_window+hub_pieces+dense_tiles_mfma"}},
        {{"spmm_csr_panel_v2", "spmm_csr_panel_v2+dense_tiles_mfma"},
         {"spmm_csr_panel_v2+hub_pieces", "spmm_csr_panel_v2+hub_pieces+dense_tiles_mfma"}}};
    return names[main][hubs ? 1 : 0][dense ? 1 : 0];
}

// Exact chains of the chain rows [c0, c1) (chain_fused, spmm_csr_kernels.h): products from the repacked B panels (segment by
// segment, like the piece kernel) and the serial sum of every (row, column) in one workgroup, epilogue included.
void launch_chains(sextans_engine *h, const std::vector<Seg> &plan, const float *dCin, int64_t ldc_in, float *dCout, int64_t ldc,
                   int N, int c0, int c1, int row_base, float alpha, float beta, hipStream_t s, bool permuted_panels = false,
                   const float *rm_B = nullptr, int64_t rm_ldb = 0) {
    // rm_B (sextans_spmm_device_rm): the caller's row-major B and C -- B is one "panel" with rows rm_ldb floats apart
    // permuted_panels (the reordered form): the 16-column panels hold B row k at row colpos[k]; the chain rows' entries come from
    // their compact relabelled copy (ensure_cluster_plan); 8-column remainder tiles keep the natural panels and the source arrays
    // one workgroup per (chain row, 16- or 8-column tile): chain_fused
    {
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
            const float *bp = rm_B ? rm_B + g.col0 : h->d_Bp + (size_t)h->K * (size_t)g.col0;
            const int NT = (g.width >= 16 && g.last_cols != 8) ? 16 : 8;   // (the tail: the first 8-column half of its 16-column panel)
            const int ntiles = g.last_cols == 8 ? 1 : g.ntiles * (g.width / NT);
            auto go = [&](auto kern, int lds, int threads) {
                (void)allow_big_lds(h, reinterpret_cast<const void *>(kern), lds);
                const bool perm = permuted_panels && g.width == 16;
                hipLaunchKernelGGL(kern, dim3((unsigned)(c1 - c0) * (unsigned)ntiles), dim3((unsigned)threads), (size_t)lds, s, h->d_chain_row,
                                   perm ? h->d_chain_beg_c : h->d_chain_beg, h->d_chain_off, (c0 == 0 && c1 == h->nchain) ? h->d_chain_perm : (const int *)nullptr,
                                   perm ? (const int *)h->d_chain_ci_perm : h->s_ci, perm ? (const float *)h->d_chain_v_c : h->s_v, bp, rm_B ? (int64_t)0 : (int64_t)h->K * g.width,
                                   rm_B ? (int)rm_ldb : g.width, dCin, ldc_in, dCout, ldc, g.col0, ntiles, c0, row_base, alpha, beta, rm_B ? 1 : 0);
            };
#define SX_FUSED(W) if (h->opt_exact) go(sx::chain_fused<W, true>, sx::chain_fused_lds_bytes(W), sx::chain_fused_threads(W)); \
                    else go(sx::chain_fused<W, false>, sx::chain_fused_lds_bytes(W), sx::chain_fused_threads(W))
            if (NT == 16) { SX_FUSED(16); } else { SX_FUSED(8); }
#undef SX_FUSED
        }
    }
}

template <int LPR>
void launch_hub_pieces(sextans_engine *h, const sextans_engine::PieceTable &t, const float *dBp, int ntiles, int col0,
                       int v0, int v1, hipStream_t s, const int *colpos = nullptr, int64_t rm_ldb = 0) {
    // rm_ldb > 0: dBp is the caller's row-major B at column col0 (sextans_spmm_device_rm)
    constexpr int RB = sx::kBlock / LPR;
    const int nblk = (v1 - v0 + RB - 1) / RB;
    if (nblk <= 0) return;
    float *P = h->d_P + (int64_t)col0 * h->split_nv;
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)nblk * (unsigned)ntiles), dim3(sx::kBlock), 0, s, t.d_vrp, t.d_vend, h->s_ci,
                           h->s_v, dBp, rm_ldb > 0 ? rm_ldb : (int64_t)h->K * 4 * LPR, P, (int64_t)h->split_nv, v0, v1, ntiles, colpos);
    };
    if (rm_ldb > 0) { if (h->opt_exact) go(sx::spmm_csr_pieces<LPR, true, true>); else go(sx::spmm_csr_pieces<LPR, false, true>); }
    else if (h->opt_exact) go(sx::spmm_csr_pieces<LPR, true>); else go(sx::spmm_csr_pieces<LPR, false>);
}

// The partial sums of the long rows [hub0, hub1) of piece table t folded in order into C (rm: the caller's row-major C)
void launch_fold(sextans_engine *h, const sextans_engine::PieceTable &t, int hub0, int hub1, int N, const float *dCin, int64_t ldc_in,
                 float *dCout, int64_t ldc, int row_base, float alpha, float beta, bool rm, hipStream_t s) {
    const int64_t tot = (int64_t)(hub1 - hub0) * N;
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, t.d_vfirst, t.d_row, h->d_P, (int64_t)h->split_nv, dCin, ldc_in,
                           dCout, ldc, hub0, hub1 - hub0, N, row_base, alpha, beta, rm ? 1 : 0);
    };
    if (h->opt_exact) go(sx::fold_hub_pieces<true>); else go(sx::fold_hub_pieces<false>);
}

// f(LPR) with the lanes per row of a tile width as a compile-time constant: 32 / 16 / 8 columns -> 8 / 4 / 2 lanes
template <class F>
int by_width(int width, F f) {
    switch (width) {
        case 32: return f(std::integral_constant<int, 8>{});
        case 16: return f(std::integral_constant<int, 4>{});
        default: return f(std::integral_constant<int, 2>{});
    }
}

// N as 32-column tiles, then at most one 16- and one 8-column tile: the launches on the caller's row-major B, whose 32-column tiles
// take whole 128-byte lines of a B row
std::vector<Seg> wide_first(int N) {
    std::vector<Seg> v;
    int col = 0;
    if (N / 32) { v.push_back(Seg{32, 0, N / 32}); col = N / 32 * 32; }
    if ((N - col) / 16) { v.push_back(Seg{16, col, 1}); col += 16; }
    if (N - col) v.push_back(Seg{8, col, 1});
    return v;
}

// Round 6 (VERDICT r05 task 2, "measure first"): how many of a block's dictionary rows does the PREVIOUS block of the walk hold too?
// One workgroup of 64 lanes per block: the previous dictionary into an LDS hash set (1024 slots, linear probing), this one probed.
// out[0] += entries of block b found in block b - 1, out[1] += entries of block b  (b >= 1).
__global__ __launch_bounds__(64) void dict_overlap(const int *__restrict__ dict_cnt, const int *__restrict__ dict, int stride, int nblk, unsigned long long *out) {
    __shared__ int tab[1024];
    const int b = (int)blockIdx.x + 1;
    if (b >= nblk) return;
    for (int i = threadIdx.x; i < 1024; i += 64) tab[i] = -1;
    __syncthreads();
    const int np = dict_cnt[b - 1], nc = dict_cnt[b];
    for (int i = threadIdx.x; i < np; i += 64) {
        const int c = dict[(int64_t)(b - 1) * stride + i];
        unsigned s = ((unsigned)c * 2654435761u) >> 22;
        while (atomicCAS(&tab[s], -1, c) != -1 && tab[s] != c) s = (s + 1) & 1023u;
    }
    __syncthreads();
    unsigned found = 0;
    for (int i = threadIdx.x; i < nc; i += 64) {
        const int c = dict[(int64_t)b * stride + i];
        unsigned s = ((unsigned)c * 2654435761u) >> 22;
        while (tab[s] != -1 && tab[s] != c) s = (s + 1) & 1023u;
        found += tab[s] == c;
    }
    for (int o = 32; o > 0; o >>= 1) found += __shfl_down(found, o);
    if (threadIdx.x == 0) { atomicAdd(&out[0], (unsigned long long)found); atomicAdd(&out[1], (unsigned long long)nc); }
}
// Share of the clustered plan's row slots that sit in runs of >= 16 consecutive rows inside their block (round 6, VERDICT r05 task 4): only
// such runs could be written to column-major C as 64-byte pieces straight from the SpMM kernel instead of through the staging buffer.
int run16_stat(sextans_engine *h, double *value) {
    *value = 0.0;
    if (h->cluster_state <= 0 || !h->d_slot_row || h->psc.plan_nblk <= 0) return SEXTANS_OK;
    const int RB = sx::kBlock / 4 * std::max(1, h->psc.plan_sets);
    std::vector<int> sr((size_t)h->psc.plan_nblk * RB);
    SX_HIP(hipMemcpy(sr.data(), h->d_slot_row, sizeof(int) * sr.size(), hipMemcpyDeviceToHost));
    const std::vector<int> &br = h->psc.h_blk_row;
    if ((int)br.size() != h->psc.plan_nblk + 1) return SEXTANS_OK;
    int64_t in_runs = 0, slots = 0;
    for (int b = 0; b < h->psc.plan_nblk; ++b) {
        const int n = br[(size_t)b + 1] - br[(size_t)b];
        const int *r = sr.data() + (size_t)b * RB;
        slots += n;
        for (int i = 0; i < n;) {
            int j = i + 1;
            while (j < n && r[j] == r[j - 1] + 1) ++j;
            if (j - i >= 16) in_runs += j - i;
            i = j;
        }
    }
    *value = slots ? (double)in_runs / (double)slots : 0.0;
    return SEXTANS_OK;
}
int dict_overlap_stat(sextans_engine *h, double *value) {
    const sextans_engine::PanelState &P = h->cluster_state > 0 ? h->psc : h->ps;
    *value = 0.0;
    if (!P.plan_built || P.plan_nblk < 2 || !P.d_dict || !P.d_dict_ptr) return SEXTANS_OK;
    unsigned long long *d = nullptr, hv[2] = {0, 0};
    SX_HIP(hipMalloc((void **)&d, sizeof hv));
    SX_HIP(hipMemset(d, 0, sizeof hv));
    hipLaunchKernelGGL(dict_overlap, dim3((unsigned)P.plan_nblk - 1), dim3(64), 0, hipStreamPerThread, P.d_dict_ptr, P.d_dict, P.plan_dict_stride, P.plan_nblk, d);
    const hipError_t e = hipMemcpy(hv, d, sizeof hv, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    SX_HIP(e);
    *value = hv[1] ? (double)hv[0] / (double)hv[1] : 0.0;
    return SEXTANS_OK;
}
}  // namespace
extern "C" {

int sextans_get_stat(sextans_handle_t h, const char *key, double *value) {
    if (!h || !key || !value) return SEXTANS_ERR_INVALID;
    if (h->d_rp) {   // figures about the packed forms refer to the current options: bring the cheap ones up to date
        SX_HIP(hipSetDevice(h->device));
        if (int rc = ensure_dense(h)) return rc;
        if (int rc = ensure_split(h)) return rc;
    }
    if (!strcmp(key, "plan_build_s")) *value = h->plan_build_s;
    else if (!strcmp(key, "window_padded_entries")) *value = (double)h->win_padded;
    else if (!strcmp(key, "window_state")) *value = (double)h->win_state;
    else if (!strcmp(key, "reassociated_rows")) *value = (double)h->h_split_rows.size();
    else if (!strcmp(key, "piece_path_rows")) *value = (double)(h->nhub + h->nchain);
    else if (!strcmp(key, "exact_chain_rows")) *value = (double)h->nchain;
    else if (!strcmp(key, "chain_threshold")) *value = (double)h->chain_T;
    else if (!strcmp(key, "split_threshold")) *value = (double)h->split_T;
    else if (!strcmp(key, "bucket_threshold")) *value = (double)h->bucket_L0;
    else if (!strcmp(key, "dense_tiles")) *value = (double)h->dense_tiles;
    else if (!strcmp(key, "dense_tile_fraction")) *value = h->nnz > 0 ? (double)h->dense_nnz / (double)h->nnz : 0.0;
    else if (!strcmp(key, "dense_tiles_on_mfma")) *value = h->dense_W > 0 ? 1.0 : 0.0;
    else if (!strcmp(key, "bell_share")) *value = h->bell_share;
    else if (!strcmp(key, "row_cluster")) *value = (double)h->cluster_state;          // 1 grid bricks / 2 graph clustering in use, -1 declined, 0 not evaluated yet
    else if (!strcmp(key, "cluster_shared_fraction")) *value = h->cluster_shared;
    else if (!strcmp(key, "cluster_decline")) *value = (double)h->cluster_decline;
    else if (!strcmp(key, "graph_fallbacks")) *value = (double)h->graph_fallbacks;   // rp_time loops launched one by one because their hipGraph capture was invalidated from outside
    else if (!strcmp(key, "cluster_run16_fraction")) return run16_stat(h, value);   // share of the clustered plan's slots in runs of >= 16 consecutive rows of their block
    else if (!strcmp(key, "dict_overlap_consecutive")) return dict_overlap_stat(h, value);   // share of a block's dictionary rows the previous block of the walk holds too (the plan whole-matrix calls use)
    else if (!strcmp(key, "dist_setup_exchanges")) *value = (double)h->dist_exchanges;   // control collectives + host syncs of the dist entry points so far (0 new ones after sextans_dist_prepare)
    else if (!strcmp(key, "cluster_graph_kind")) *value = (double)h->cluster_graph_kind;
    else if (!strcmp(key, "cluster_runs")) *value = h->cluster_runs ? 1.0 : 0.0;
    else if (!strcmp(key, "pattern_symmetry")) *value = h->pattern_symmetry;
    else if (!strcmp(key, "col_range_lo")) *value = (double)h->col_lo;
    else if (!strcmp(key, "col_range_hi")) *value = (double)h->col_hi;
    else if (!strcmp(key, "b_rows_repacked")) *value = h->d_touched ? (double)h->touched_segments * 64.0 : (double)(h->col_hi - h->col_lo);
    else if (!strcmp(key, "colwise")) *value = (double)h->colwise_state;
    else if (!strcmp(key, "mixed_plan")) *value = h->ps.plan_built && h->ps.plan_mixed ? (h->ps.d_rg_skip && h->opt_split_mixed != 0 ? 2.0 : 1.0) : 0.0;   // 2: runs in its split form
    else if (!strcmp(key, "row_sets")) *value = (double)(h->cluster_state > 0 ? h->psc.plan_sets : h->ps.plan_sets);
    else if (!strcmp(key, "row_coherence")) *value = h->row_coherence;
    else if (!strcmp(key, "panel_blocks_clustered")) *value = (double)h->psc.plan_nblk;
    else if (!strcmp(key, "device_bytes")) *value = (double)device_bytes(h);
    else if (!strcmp(key, "value_refreshes")) *value = (double)h->value_refreshes;                  // sextans_update_values* served on this matrix
    else if (!strcmp(key, "value_refresh_rebuilt")) *value = (double)h->value_refresh_rebuilt;      //   ... that dropped a form for a lazy rebuild
    else if (!strcmp(key, "bf16_native_calls")) *value = (double)(h->bf16_native_calls + (h->tr ? h->tr->bf16_native_calls : 0));            // bf16 calls (transposed ones included) on the caller's buffers
    else if (!strcmp(key, "bf16_converted_calls")) *value = (double)(h->bf16_converted_calls + (h->tr ? h->tr->bf16_converted_calls : 0));   //   ... and through fp32 copies
    else if (!strcmp(key, "transpose_build_s")) *value = h->transpose_build_s + (h->tr ? h->tr->plan_build_s : 0.0);
    else if (!strcmp(key, "grid_stride_line")) *value = (double)h->cluster_s2;
    else if (!strcmp(key, "grid_stride_plane")) *value = (double)h->cluster_s3;
    else if (!strcmp(key, "panel_rows_natural")) *value = (double)h->plan_total_dict;  // B rows copied into LDS per N tile, natural order
    else if (!strcmp(key, "panel_rows_clustered")) *value = (double)h->cluster_total_dict;
    else if (!strcmp(key, "panel_fraction")) *value = h->ps.plan_panel_frac;
    else if (!strcmp(key, "panel_blocks")) *value = (double)h->ps.plan_nblk;
    else if (!strcmp(key, "index_stream_entries")) *value = (double)(h->cluster_state > 0 ? h->psc.plan_idx_len : h->ps.plan_idx_len);
    else if (!strcmp(key, "value_stream_entries")) *value = (double)(h->cluster_state > 0 ? h->psc.plan_stream_len : h->ps.plan_stream_len);
    else return SEXTANS_ERR_INVALID;
    return SEXTANS_OK;
}

int sextans_export_plan(sextans_handle_t h, int lanes_per_row, sextans_packed *out) {
    if (!h || !out || (lanes_per_row != 2 && lanes_per_row != 4 && lanes_per_row != 8)) return SEXTANS_ERR_INVALID;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    SX_HIP(hipSetDevice(h->device));
    if (int rc = ensure_dense(h)) return rc;
    if (int rc = ensure_split(h)) return rc;
    if (int rc = ensure_plan(h, lanes_per_row, true)) return rc;
    if (!h->ps.plan_built) return SEXTANS_ERR_STATE;
    if (int rc = restore_plan_streams(h)) return rc;
    const auto &ps = h->ps;
    const int M = h->M, nblk = ps.plan_nblk, RB = sx::kBlock / lanes_per_row;
    const size_t L = (size_t)ps.plan_stream_len;
    memset(out, 0, sizeof *out);
    out->M = M; out->K = h->K; out->nnz = h->m_nnz; out->lanes_per_row = lanes_per_row; out->nblk = nblk;
    out->stream_len = (int64_t)L; out->max_dict = ps.plan_max_dict; out->nnz_in_panel_blocks = ps.plan_nnz_panel;
    std::vector<int> rp((size_t)M + 1), cnt((size_t)nblk), bd((size_t)nblk * ps.plan_dict_stride);
    SX_HIP(hipMemcpy(rp.data(), h->m_rp, sizeof(int) * rp.size(), hipMemcpyDeviceToHost));
    if (nblk) {
        SX_HIP(hipMemcpy(cnt.data(), ps.d_dict_ptr, sizeof(int) * cnt.size(), hipMemcpyDeviceToHost));
        SX_HIP(hipMemcpy(bd.data(), ps.d_dict, sizeof(int) * bd.size(), hipMemcpyDeviceToHost));
    }
#define SX_HIP_OUT(call) do { if ((call) != hipSuccess) { g_last_error = #call; (void)hipGetLastError(); sextans_packed_free(out); return SEXTANS_ERR_HIP; } } while (0)   /* (no leak of the arrays allocated above) */
    auto alloc = [](size_t bytes) { return calloc(bytes ? bytes : 1, 1); };
    out->blk_row = (int *)alloc(sizeof(int) * ((size_t)nblk + 1));
    out->dict_ptr = (int *)alloc(sizeof(int) * ((size_t)nblk + 1));
    out->row_off = (int *)alloc(sizeof(int) * ((size_t)M + 1));
    out->idx16 = (uint16_t *)alloc(sizeof(uint16_t) * L);
    out->col32 = (int *)alloc(sizeof(int) * L);
    out->val = (float *)alloc(sizeof(float) * L);
    size_t ndict = 0;
    for (int b = 0; b < nblk; ++b) ndict += (size_t)cnt[(size_t)b];
    out->dict = (int *)alloc(sizeof(int) * ndict);
    if (!out->blk_row || !out->dict_ptr || !out->row_off || !out->idx16 || !out->col32 || !out->val || !out->dict) {
        sextans_packed_free(out);
        return SEXTANS_ERR_ALLOC;
    }
    memcpy(out->blk_row, ps.h_blk_row.data(), sizeof(int) * ((size_t)nblk + 1));
    size_t w = 0;
    for (int b = 0; b < nblk; ++b) {
        out->dict_ptr[b] = (int)w;
        for (int i = 0; i < cnt[(size_t)b]; ++i) out->dict[w++] = bd[(size_t)b * ps.plan_dict_stride + (size_t)i];
    }
    out->dict_ptr[nblk] = (int)w;
    for (int r = 0; r < M; ++r) out->row_off[r + 1] = out->row_off[r] + ((rp[(size_t)r + 1] - rp[(size_t)r] + 3) & ~3);
    if (!ps.d_ioff) {
        SX_HIP_OUT(hipMemcpy(out->idx16, ps.d_lidx, sizeof(uint16_t) * L, hipMemcpyDeviceToHost));
    } else {   // index lists shared between consecutive rows: the public form carries every row's own list
        std::vector<uint16_t> comp((size_t)ps.plan_idx_len);
        std::vector<int> ioff((size_t)nblk * RB * 2), sinfo((size_t)nblk * RB * 2);
        SX_HIP_OUT(hipMemcpy(comp.data(), ps.d_lidx, sizeof(uint16_t) * comp.size(), hipMemcpyDeviceToHost));
        SX_HIP_OUT(hipMemcpy(ioff.data(), ps.d_ioff, sizeof(int) * ioff.size(), hipMemcpyDeviceToHost));
        SX_HIP_OUT(hipMemcpy(sinfo.data(), ps.d_row_off, sizeof(int) * sinfo.size(), hipMemcpyDeviceToHost));
        const unsigned pad = (unsigned)ps.plan_pad_row * 16u * (unsigned)lanes_per_row;
        for (size_t i = 0; i < (size_t)nblk * RB; ++i) {
            const int o0 = sinfo[2 * i], len = sinfo[2 * i + 1], src = ioff[2 * i], shift = ioff[2 * i + 1];
            for (int e = 0; e < len; ++e) {
                const unsigned v = comp[(size_t)src + e];
                out->idx16[(size_t)o0 + e] = (uint16_t)(v == pad ? v : v + (unsigned)shift);
            }
        }
    }
    SX_HIP_OUT(hipMemcpy(out->val, ps.d_pval, sizeof(float) * L, hipMemcpyDeviceToHost));
    if (ps.plan_mixed) SX_HIP_OUT(hipMemcpy(out->col32, ps.d_pcol32, sizeof(int) * L, hipMemcpyDeviceToHost));
    // device stream: byte offset of the B row in the panel; public form: dictionary index, 0xFFFF in the padding
    const unsigned row_bytes = 16u * (unsigned)lanes_per_row, pad_off = (unsigned)ps.plan_pad_row * row_bytes;
    for (size_t i = 0; i < L; ++i) out->idx16[i] = out->idx16[i] == pad_off ? (uint16_t)0xFFFF : (uint16_t)(out->idx16[i] / row_bytes);
    (void)RB;
    return SEXTANS_OK;
#undef SX_HIP_OUT
}

int sextans_reassociated_rows(sextans_handle_t h, int *rows, int capacity, int *count) {
    if (!h || !count || capacity < 0 || (capacity > 0 && !rows)) return SEXTANS_ERR_INVALID;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    SX_HIP(hipSetDevice(h->device));
    if (int rc = ensure_dense(h)) return rc;
    if (int rc = ensure_split(h)) return rc;
    *count = (int)h->h_split_rows.size();
    for (int i = 0; i < *count && i < capacity; ++i) rows[i] = h->h_split_rows[(size_t)i];
    return SEXTANS_OK;
}

}  // extern "C"
namespace {
// One SpMM as the caller asked for it: operands, row range [row_begin, row_end) (whole: all of the matrix), flags, stream
struct Call {
    int N; float alpha; const float *B; int64_t ldb; float beta; const float *C_in; int64_t ldc_in; float *C_out; int64_t ldc;
    int row_begin, row_end, flags; hipStream_t s; bool whole;
};

// The chains need one or two wavefronts for about a millisecond: on their own stream, beside the main kernel (fork after the B
// panels are in place, join before the call's work on `s` is considered complete).  rm: from the caller's row-major B.
int fork_chains(sextans_engine *h, const Call &c, const std::vector<Seg> &segs, int ch0, int ch1, bool rm) {
    SX_HIP(hipEventRecord(h->ev_fork, c.s));
    SX_HIP(hipStreamWaitEvent(h->aux_stream, h->ev_fork, 0));
    launch_chains(h, segs, c.C_in, c.ldc_in, c.C_out, c.ldc, c.N, ch0, ch1, c.row_begin, c.alpha, c.beta, h->aux_stream, false,
                  rm ? c.B : nullptr, rm ? c.ldb : 0);
    SX_HIP(hipEventRecord(h->ev_join, h->aux_stream));
    return SEXTANS_OK;
}

// Everything sextans_spmm_device_rows decides for one call (route_cm), before anything is launched
struct RouteCM {
    enum Path { kWindow, kColwise, kSegments } path = kSegments;
    enum Launch { kReorderedV2, kV2Wide, kSplitMixed, kV2, kPanel, kRowgroup };   // of a segment; the first four are spmm_csr_panel_v2
    bool panel = false;                                // the plan's panel kernels serve this range: its row blocks [blk0, blk1)
    int blk0 = 0, blk1 = 0;
    const sextans_engine::PieceTable *pt = nullptr;    // long rows of this range: entries [hub0, hub1) of *pt, pieces [v0, v1)
    int hub0 = 0, hub1 = 0, v0 = 0, v1 = 0;
    int ch0 = 0, ch1 = 0;                              // chain rows of this range
    bool hubs = false, chains = false;
    bool fuse_b = false, reordered = false, clustered = false;
    int64_t cs_tile = 0;                               // reordered: floats per 16-column tile of the staging buffer
    std::vector<Seg> segs;                             // the tiling of N, its 8-column tail merged where that pays
    Launch launch[3] = {};                             // per segment (at most three: tiles W, 16 and 8 columns wide)
    int layout = 0;                                    // bp_layout of the panels this call runs on
    bool skip_repack = false;
};

// The launch of every segment of r.segs (W: the width the plan is built for; wide_fits_b: route_cm)
void choose_launches(const sextans_engine *h, const Call &c, int W, bool wide_fits_b, RouteCM &r) {
    // (column-major staging keeps the round-1 kernel unless the rows are short: then the register-resident form fits
    // 128 registers together with a panel in registers)
    const bool short_rows = h->M > 0 && h->m_nnz / h->M + 8 <= 32;
    for (size_t i = 0; i < r.segs.size(); ++i) {
        const Seg &g = r.segs[i];
        const bool panel_here = r.panel && g.width == W;   // the plan is built for width W
        const bool v2_16 = panel_here && g.width == 16 && wide_fits_b;
        // (long rows + column-major staging: the 256-register instantiation, for launches that cannot fill the chip -- option
        // "panel_v2" = 1 asks for it, the automatic setting keeps spmm_csr_panel there: measured)
        const bool big_ok = r.fuse_b && !short_rows && h->opt_panel_v2 == 1 && (int64_t)(r.blk1 - r.blk0) * g.ntiles <= 8192;
        RouteCM::Launch l = panel_here ? RouteCM::kPanel : RouteCM::kRowgroup;
        if (r.reordered && g.width == 16) l = RouteCM::kReorderedV2;
        // N >= 32 on a dictionary-only plan at 4 lanes per row: register-blocked 32-column super tiles with the
        // tile loop inside the workgroup; an odd 16-column tile at the end goes to the plain panel kernel
        else if (v2_16 && !h->ps.plan_mixed && h->opt_cols_per_lane == 8 && g.ntiles >= 2) l = RouteCM::kV2Wide;
        // MIXED plans, split form (round 5): the blocks that have a dictionary run on the register-resident kernel (it leaves the others
        // alone), the rows of the blocks without one -- no reuse between their rows -- on the gather kernel behind it (its skip table
        // names the rows that are not its own).  One launch of spmm_csr_panel<MIXED> did both at the speed of neither: FEM rows + 10 / 30 /
        // 60 % uniformly random rows, N = 16: 311 / 468 / 698 us per step -> 280 / 424 / 644; through the row-major entry point 406 / 581 / 832
        // (column-major copies around the mixed kernel) -> 235 / 375 / 611 (tools/mixed_rm_probe.py).  Both launches walk compact lists
        // (blocks with a dictionary; groups of 128 rows with a gather row): a launch over everything whose other workgroups leave at
        // once hands the XCDs unequal shares -- measured 2 x slower.  (The gather launch on a second stream beside the other one: built,
        // measured equal -- the first launch fills every workgroup slot of the chip, the second queues behind it either way.)
        // (whole-matrix calls: the launches walk lists made for the whole plan)
        else if (v2_16 && h->ps.plan_mixed && h->ps.d_rg_skip && h->opt_split_mixed != 0 && h->opt_panel_v2 != 0 && !r.fuse_b &&
                 h->opt_kernel == 0 && c.whole) l = RouteCM::kSplitMixed;
        else if (v2_16 && !h->ps.plan_mixed && h->opt_panel_v2 != 0 && (!r.fuse_b || short_rows || big_ok)) l = RouteCM::kV2;
        r.launch[i] = l;
    }
}

RouteCM route_cm(const sextans_engine *h, const Call &c, Tiling t) {
    RouteCM r;
    const int N = c.N;
    // a row range keeps the panel kernel when it starts and ends on row-block boundaries of the plan
    r.panel = t.panel;
    r.blk1 = h->ps.plan_nblk;
    if (r.panel && !c.whole) {
        const auto &br = h->ps.h_blk_row;
        const auto i0 = std::lower_bound(br.begin(), br.end(), c.row_begin), i1 = std::lower_bound(br.begin(), br.end(), c.row_end);
        if (i0 == br.end() || *i0 != c.row_begin || i1 == br.end() || *i1 != c.row_end) r.panel = false;
        else { r.blk0 = (int)(i0 - br.begin()); r.blk1 = (int)(i1 - br.begin()); }
    }
    // ... and the window kernel when it starts and ends on wavefront (rows-per-wave) boundaries
    const bool window = t.window && c.row_begin % h->win_rw == 0 && (c.row_end % h->win_rw == 0 || c.row_end == h->M);
    // long rows of this range: entries [hub0, hub1) of a piece table, pieces [v0, v1).  Whole-matrix calls walk the
    // table sorted by length (workgroups of equally long pieces), row ranges the one sorted by row.
    r.pt = c.whole ? &h->by_len : &h->by_row;
    if (h->nhub > 0) {
        const auto &rows = r.pt->h_row;
        if (c.whole) { r.hub1 = h->nhub; }
        else {
            r.hub0 = (int)(std::lower_bound(rows.begin(), rows.end(), c.row_begin) - rows.begin());
            r.hub1 = (int)(std::lower_bound(rows.begin(), rows.end(), c.row_end) - rows.begin());
        }
        r.v0 = r.pt->h_vfirst[(size_t)r.hub0]; r.v1 = r.pt->h_vfirst[(size_t)r.hub1];
    }
    r.hubs = r.hub1 > r.hub0;
    r.ch1 = h->nchain;
    if (h->nchain > 0 && !c.whole) {
        r.ch0 = (int)(std::lower_bound(h->h_chain_row.begin(), h->h_chain_row.end(), c.row_begin) - h->h_chain_row.begin());
        r.ch1 = (int)(std::lower_bound(h->h_chain_row.begin(), h->h_chain_row.end(), c.row_end) - h->h_chain_row.begin());
    }
    r.chains = r.ch1 > r.ch0;
    if (window) {
        // (a reuse request is honoured only if the panels in the workspace have this layout: row-range calls of
        // one pipelined SpMM may alternate between the window kernel's 8-column panels and those of the other kernels)
        r.path = RouteCM::kWindow;
        r.layout = 8;
        r.skip_repack = (c.flags & SEXTANS_ROWS_REUSE_B_PANELS) != 0 && h->bp_layout == 8;
        return r;
    }
    // Short rows in a numbering with locality (or "kernel" = 4): one lane per row on the caller's column-major operands -- no B
    // repack, no LDS (spmm_colwise_kernel.h).  Rows on the long-row paths need the repacked panels: then the other kernels run.
    if (colwise_wanted(h) && !r.hubs && !r.chains && csr_only(h) && h->m_nnz > 0) {
        r.path = RouteCM::kColwise;
        return r;
    }
    // Small B (fits the L2s), dictionary-only plan, one N segment: the panel kernel stages straight from the
    // caller's column-major B and the repack launch disappears.
    r.fuse_b = r.panel && !h->ps.plan_mixed && h->opt_fuse_b && !(c.flags & kRowsNoFuseB) && t.segs.size() == 1 && h->rb_n == 0 &&   // (routed row blocks read the repacked panels)
               t.segs[0].width == t.W && !r.hubs && !r.chains &&
               (size_t)h->K * (size_t)N * sizeof(float) <= ((size_t)16 << 20) &&
               // (a graph-clustered plan beats the natural-order blocks of a renumbered matrix also while B fits the L2s, once the
               // matrix is large enough for three more launches not to matter: 332 K rows 123 -> 85 us per step)
               // (... and below that size once the call is large enough: a 13 965-row matrix in a random node order, N = 128,
               // 112 us staged from column-major B on its natural-order plan against 34 us reordered; N = 16: 13.3 against 15.0.
               // Crossover measured at ~24 M non-zero x column products: tools/small_renumbered.py)
               !(c.whole && h->cluster_state == 2 && h->cluster_cm_pays && (h->M >= 65536 || h->m_nnz * (int64_t)N >= ((int64_t)24 << 20)));
    // (Staging from column-major B for LARGE matrices -- no repack launch at all -- was measured in round 4 and loses everywhere: 4M-row
    // 3-dof FEM N = 16 kernel 660 -> 872 us against 83 us of repack saved; 1-dof 27-point 379 -> 577; 2-D 9-point 296 -> 427;
    // 5-point 270 -> 412: 36 four-byte loads per lane and panel through registers instead of nine LDS-DMA requests.)
    // The reordered form (graph-clustered plan, ensure_cluster_plan): whole-matrix calls, 16-column tiles.  Its B panels hold the
    // rows of B in the plan's column order and C goes through the block-major staging buffer (reorder_kernels.h); an 8-column
    // remainder tile keeps the natural-order kernels and panels.  (Layout tag -W: such panels are never reused by a row-range call.)
    r.reordered = c.whole && h->cluster_state == 2 && h->cluster_cm_pays && h->opt_kernel != 1 && h->opt_kernel != 3 && t.W == 16 && !r.fuse_b &&
                  (!r.chains || h->d_chain_ci_perm) && csr_only(h) && h->d_Cs &&
                  // (the staging buffer is sized by prepare() for the N it saw: a plan that survived a set_option("kernel") and a
                  // larger N since then must not run past its end -- ADVICE r04)
                  h->Cs_cap >= (size_t)((N + 15) / 16) * (size_t)h->M * 16 && (N >= 16 || (N == 8 && !r.hubs && !r.chains));
    r.cs_tile = r.reordered ? (int64_t)h->M * 16 : 0;
    // 32-bit byte offsets inside the wide kernels: panels and C columns (wide_fits), and the caller's B when the kernel stages
    // from it (wide_fits_b)
    const bool wide_fits = h->ps.plan_max_dict <= sx::kWideMaxDict && (int64_t)h->K * 64 < ((int64_t)1 << 32) &&
                           std::max(c.ldc, c.ldc_in) * 64 < ((int64_t)1 << 32);
    const bool wide_fits_b = wide_fits && (!r.fuse_b || c.ldb * 64 < ((int64_t)1 << 32));
    // N = 16 t + 8 on the register-resident panel kernel: the 8-column tail used to go to the gather kernel (the plan is built for
    // 16-column tiles) -- 4M-row FEM matrix: N = 24 2 152 us per step against 1 099 at N = 32.  It now runs as one more 16-column tile:
    // its B panel is zero in the 8 columns that do not exist, the kernel neither loads nor stores C there (`last_cols`), the passes of
    // the reordered form skip them; rows on the piece path sum 16 columns into their (wider) partial-sum buffer and fold N, the exact
    // chains take the tail as one 8-column tile of the 16-column panel.  Not with dense tiles on the MFMA path or column-major staging.
    const bool v2 = r.reordered || (r.panel && !h->ps.plan_mixed && h->opt_panel_v2 != 0 && !r.fuse_b && wide_fits && h->opt_cols_per_lane != 8);
    std::vector<Seg> &plan = r.segs;
    plan = std::move(t.segs);
    if (v2 && t.W == 16 && plan.size() == 2 && plan[0].width == 16 && plan[1].width == 8 && plan[1].ntiles == 1 &&
        (h->nhub == 0 || h->P_cap >= (size_t)h->split_nv * (size_t)(N + 8)) &&
        // (with rows on the piece / chain paths only where the main rows are long enough to matter: on the KKT class -- 6 entries per
        // row, arrow borders as chains -- the wider piece / chain work cost more than the gather tail: 1 510 -> 1 687 us at N = 24)
        ((h->nhub == 0 && h->nchain == 0) || (h->M > 0 && h->m_nnz / h->M >= 16)) &&
        csr_only(h) && h->Bp_cap >= (size_t)h->K * (size_t)(N + 8) &&
        (!r.reordered || h->Cs_cap >= (size_t)(N / 16 + 1) * (size_t)h->M * 16)) {
        plan[0].ntiles += 1;
        plan[0].last_cols = 8;
        plan.pop_back();
    } else if (v2 && t.W == 16 && plan.size() == 1 && plan[0].width == 8 && plan[0].ntiles == 1 && h->nhub == 0 && h->nchain == 0 &&
               csr_only(h) && h->Bp_cap >= (size_t)h->K * 16 && (!r.reordered || h->Cs_cap >= (size_t)h->M * 16)) {
        plan[0] = Seg{16, 0, 1, 8};   // N = 8 on the 16-column plan (engine_plan.hip: prepare, n8_wide)
    }
    r.layout = r.reordered ? -t.W : plan[0].last_cols != 0 ? t.W + 100 : t.W;
    r.skip_repack = r.fuse_b || ((c.flags & SEXTANS_ROWS_REUSE_B_PANELS) != 0 && h->bp_layout == r.layout);
    // whole-matrix calls on repacked panels: the plan over the rows in clustered (brick) order when the matrix has one
    r.clustered = c.whole && !r.fuse_b && h->cluster_state == 1;
    choose_launches(h, c, t.W, wide_fits_b, r);
    return r;
}

int run_window(sextans_engine *h, const Call &c, const RouteCM &r) {
    const int N = c.N;
    hipStream_t s = c.s;
    // B in 8-column panels (the reference's N tile), then one tile-major launch
    if (!r.skip_repack) {
        Prof p(h, &h->ev_repack, s);
        launch_repack<8>(c.B, c.ldb, h->d_Bp, h->K, 0, N / 8, s, h->col_lo, h->col_hi, -1, h->d_touched);
        h->bp_layout = r.layout;
    }
    {
        Prof p(h, &h->ev_kernel, s);
        const int w0 = c.row_begin / h->win_rw, w1 = (c.row_end + h->win_rw - 1) / h->win_rw;
        launch_window(h, h->d_Bp, c.C_in, c.ldc_in, c.C_out, c.ldc, N / 8, w0, w1, c.row_begin, c.alpha, c.beta, s);
        const std::vector<Seg> p8{{8, 0, N / 8}};
        if (r.hubs) {
            launch_hub_pieces<2>(h, *r.pt, h->d_Bp, N / 8, 0, r.v0, r.v1, s);
            launch_fold(h, *r.pt, r.hub0, r.hub1, N, c.C_in, c.ldc_in, c.C_out, c.ldc, c.row_begin, c.alpha, c.beta, false, s);
        }
        if (r.chains) launch_chains(h, p8, c.C_in, c.ldc_in, c.C_out, c.ldc, N, r.ch0, r.ch1, c.row_begin, c.alpha, c.beta, s);
        h->last_kernel = kernel_name(2, r.hubs || r.chains, h->dense_W > 0);
        if (h->rb_n > 0) {
            if (int rc = launch_rowblocks(h, p8, c.C_in, c.ldc_in, c.C_out, c.ldc, N, c.row_begin, c.row_end, c.alpha, c.beta, s)) return rc;
            h->last_kernel = with_rowblocks(h, h->last_kernel);
        }
    }
    SX_HIP(hipGetLastError());
    return SEXTANS_OK;
}

int run_colwise(sextans_engine *h, const Call &c) {
    Prof p(h, &h->ev_kernel, c.s);
    const int nrowblk = (c.row_end - c.row_begin + sx::kBlock - 1) / sx::kBlock;
    auto go = [&](auto kern, int col0, int ntiles) {
        // (tiles of a row block neighbours in the launch order: the row block's CSR entries come from HBM once -- measured on the 4M-row
        // 5-point stencil, two boxes: N = 32 0.513 / 0.527 -> 0.532 / 0.550 of the roofline; N = 48 / 64 equal or 1 % behind; N = 128 / 256
        // 0.51 -> 0.43 .. 0.49: more column streams in flight per XCD than its L2 keeps; "colwise_tiles_adjacent" 1 = two tiles, 2 = always,
        // 0 = never; profiles/r05_colwise_tile_order_ab.txt)
        const int adj = ntiles > 1 && (h->opt_colwise_tiles_adjacent == 2 || (h->opt_colwise_tiles_adjacent == 1 && ntiles <= 2)) &&
                        (int64_t)nrowblk * ntiles < ((int64_t)1 << 31) ? ntiles : 0;
        hipLaunchKernelGGL(kern, adj ? dim3((unsigned)nrowblk * (unsigned)ntiles) : dim3((unsigned)nrowblk, (unsigned)ntiles), dim3(sx::kBlock), 0, c.s, h->m_rp, h->m_ci,
                           h->m_v, c.B, c.ldb, c.C_in, c.ldc_in, c.C_out, c.ldc, c.row_begin, c.row_end, nrowblk, col0, c.alpha, c.beta, (int)h->opt_xcd,
                           (const unsigned char *)h->d_skip, adj, 1);
    };
    const int n16 = c.N / 16;
    if (n16 > 0) { if (h->opt_exact) go(sx::spmm_csr_colwise<true, 16>, 0, n16); else go(sx::spmm_csr_colwise<false, 16>, 0, n16); }
    if (c.N % 16) { if (h->opt_exact) go(sx::spmm_csr_colwise<true, 8>, n16 * 16, 1); else go(sx::spmm_csr_colwise<false, 8>, n16 * 16, 1); }
    h->last_kernel = "spmm_csr_colwise";
    SX_HIP(hipGetLastError());
    return SEXTANS_OK;
}

// One segment's main launch(es) and, for rows on the piece path, its piece launch
int launch_segment(sextans_engine *h, const Call &c, const RouteCM &r, const Seg &g, RouteCM::Launch l) {
    hipStream_t s = c.s;
    const float *bp = h->d_Bp + (size_t)h->K * (size_t)g.col0;
    const float *cin = c.C_in + (int64_t)g.col0 * c.ldc_in;
    float *cout = c.C_out + (int64_t)g.col0 * c.ldc;
    const float *bsrc = r.fuse_b ? c.B + (int64_t)g.col0 * c.ldb : bp;
    const int64_t bld = r.fuse_b ? c.ldb : 0;
    switch (l) {
        case RouteCM::kReorderedV2:
            if (int rc = launch_panel_v2<1>(h, bp, h->d_Cs, r.cs_tile, h->d_Cs, r.cs_tile, g.ntiles, c.alpha, c.beta, s, 0, 0, h->psc.plan_nblk, 0, 2))
                return rc;   // (a merged tail tile needs no mask here: its staging columns exist, the pass below writes back the valid ones)
            // rows on the piece path: their partial sums from the PERMUTED panels (column c sits at row colpos[c]); folded into C
            // behind the staging -> C pass below, which leaves C_in in their rows
            if (r.hubs) launch_hub_pieces<4>(h, *r.pt, bp, g.ntiles, g.col0, r.v0, r.v1, s, h->d_colpos);
            return SEXTANS_OK;
        case RouteCM::kV2Wide: {
            const int nsuper = g.ntiles / 2;
            if (int rc = launch_panel_v2<2>(h, bsrc, cin, c.ldc_in, cout, c.ldc, nsuper, c.alpha, c.beta, s, bld, r.blk0, r.blk1, c.row_begin))
                return rc;
            if (g.ntiles & 1) {
                const int64_t c0 = (int64_t)nsuper * 32;
                if (int rc = launch_panel<4>(h, r.fuse_b ? bsrc + c0 * c.ldb : bsrc + c0 * (int64_t)h->K, cin + c0 * c.ldc_in, c.ldc_in,
                                             cout + c0 * c.ldc, c.ldc, 1, c.alpha, c.beta, s, bld, r.blk0, r.blk1, c.row_begin))
                    return rc;
            }
            break;
        }
        case RouteCM::kSplitMixed:
            if (int rc = launch_panel_v2<1>(h, bsrc, cin, c.ldc_in, cout, c.ldc, g.ntiles, c.alpha, c.beta, s, 0, r.blk0, r.blk1, c.row_begin, 0, 16, 0, true))
                return rc;
            launch_rowgroup<4>(h, h->m_rp, h->m_rp + 1, h->m_ci, h->m_v, false, h->ps.d_rg_skip, bp, cin, c.ldc_in, cout, c.ldc, c.row_begin, c.row_end, g.ntiles,
                               c.alpha, c.beta, s, 0, false, h->ps.d_rg_groups, h->ps.rg_ngroups);
            break;
        case RouteCM::kV2:
            if (int rc = launch_panel_v2<1>(h, bsrc, cin, c.ldc_in, cout, c.ldc, g.ntiles, c.alpha, c.beta, s, bld, r.clustered ? 0 : r.blk0,
                                            r.clustered ? h->psc.plan_nblk : r.blk1, c.row_begin, r.clustered ? 1 : 0, g.last_cols ? g.last_cols : 16))
                return rc;
            break;
        default:   // the panel or the gather kernel at the lanes per row of the segment's width
            return by_width(g.width, [&](auto L) -> int {
                constexpr int LPR = decltype(L)::value;
                if (l == RouteCM::kPanel) {
                    if (int rc = launch_panel<LPR>(h, bsrc, cin, c.ldc_in, cout, c.ldc, g.ntiles, c.alpha, c.beta, s, bld, r.blk0, r.blk1, c.row_begin)) return rc;
                } else {
                    launch_rowgroup<LPR>(h, h->m_rp, h->m_rp + 1, h->m_ci, h->m_v, false, h->d_skip, bp, cin, c.ldc_in, cout, c.ldc, c.row_begin, c.row_end,
                                         g.ntiles, c.alpha, c.beta, s);
                }
                if (r.hubs) launch_hub_pieces<LPR>(h, *r.pt, bp, g.ntiles, g.col0, r.v0, r.v1, s);
                return SEXTANS_OK;
            });
    }
    if (r.hubs) launch_hub_pieces<4>(h, *r.pt, bp, g.ntiles, g.col0, r.v0, r.v1, s);
    return SEXTANS_OK;
}

int run_segments(sextans_engine *h, const Call &c, const RouteCM &r) {
    const int N = c.N;
    hipStream_t s = c.s;
    auto seg_cols = [](const Seg &g) { return g.last_cols ? (g.ntiles - 1) * g.width + g.last_cols : g.ntiles * g.width; };
    if (!r.skip_repack || r.reordered) {
        Prof p(h, &h->ev_repack, s);
        if (!r.skip_repack) {
            h->bp_layout = r.layout;
            for (const Seg &g : r.segs) {
                float *dst = h->d_Bp + (size_t)h->K * (size_t)g.col0;
                if (r.reordered && g.width == 16 && h->d_colpos) {
                    hipLaunchKernelGGL(sx::repack_b_panels_perm, dim3((unsigned)((h->col_hi - h->col_lo + sx::kBlock - 1) / sx::kBlock), (unsigned)g.ntiles),
                                       dim3(sx::kBlock), 0, s, c.B, c.ldb, dst, h->K, g.col0, h->d_colpos, h->col_lo, h->col_hi, seg_cols(g), h->d_touched);
                    continue;
                }
                by_width(g.width, [&](auto L) {   // (panels of the segment's width: 4 * LPR columns)
                    launch_repack<4 * decltype(L)::value>(c.B, c.ldb, dst, h->K, g.col0, g.ntiles, s, h->col_lo, h->col_hi, seg_cols(g), h->d_touched);
                    return SEXTANS_OK;
                });
            }
        }
        if (r.reordered)
            for (const Seg &g : r.segs)
                if (g.width == 16)
                    launch_repack<16>(c.C_in, c.ldc_in, h->d_Cs, h->M, g.col0, g.ntiles, s, 0, -1, seg_cols(g));   // C_in -> row-major tiles
    }
    {
        Prof p(h, &h->ev_kernel, s);
        if (r.chains && !r.reordered)
            if (int rc = fork_chains(h, c, r.segs, r.ch0, r.ch1, false)) return rc;
        for (size_t i = 0; i < r.segs.size(); ++i)
            if (int rc = launch_segment(h, c, r, r.segs[i], r.launch[i])) return rc;
        if (r.hubs && !r.reordered) launch_fold(h, *r.pt, r.hub0, r.hub1, N, c.C_in, c.ldc_in, c.C_out, c.ldc, c.row_begin, c.alpha, c.beta, false, s);
        if (r.chains && !r.reordered) SX_HIP(hipStreamWaitEvent(s, h->ev_join, 0));
        const bool v2_used = std::any_of(r.launch, r.launch + r.segs.size(), [](RouteCM::Launch l) { return l < RouteCM::kPanel; });
        h->last_kernel = r.reordered ? "spmm_csr_panel_v2_reordered" : kernel_name(v2_used ? 3 : r.panel ? 1 : 0, r.hubs || r.chains, h->dense_W > 0);
        if (h->rb_n > 0) {   // dense blocks of 16 rows on the fp32 matrix cores, from the same panels (the kernels above skipped their rows)
            if (int rc = launch_rowblocks(h, r.segs, c.C_in, c.ldc_in, c.C_out, c.ldc, N, c.row_begin, c.row_end, c.alpha, c.beta, s)) return rc;
            h->last_kernel = with_rowblocks(h, h->last_kernel);
        }
    }
    if (r.reordered) {
        Prof p(h, &h->ev_post, s);
        for (const Seg &g : r.segs)
            if (g.width == 16)
                hipLaunchKernelGGL(sx::tiles_to_colmajor, dim3((unsigned)((h->M + sx::kBlock - 1) / sx::kBlock), (unsigned)g.ntiles),
                                   dim3(sx::kBlock), 0, s, h->d_Cs, c.C_out, c.ldc, h->M, g.col0, seg_cols(g));
        if (r.hubs) launch_fold(h, *r.pt, r.hub0, r.hub1, N, c.C_in, c.ldc_in, c.C_out, c.ldc, c.row_begin, c.alpha, c.beta, false, s);
        // chain rows write C themselves: behind the staging -> C pass (which left C_in in their rows), from the permuted panels
        if (r.chains) launch_chains(h, r.segs, c.C_in, c.ldc_in, c.C_out, c.ldc, N, r.ch0, r.ch1, c.row_begin, c.alpha, c.beta, s, true);
    }
    SX_HIP(hipGetLastError());
    return SEXTANS_OK;
}
}  // namespace
extern "C" {

int sextans_spmm_device_rows(sextans_handle_t h, int N, float alpha, const float *d_B, int64_t ldb,
                             float beta, const float *d_C_in, int64_t ldc_in, float *d_C_out, int64_t ldc,
                             int row_begin, int row_end, int flags, void *stream) {
    if (!h || N <= 0 || (N % 8) != 0 || !d_B || !d_C_in || !d_C_out) return SEXTANS_ERR_INVALID;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    if (row_begin < 0 || row_end < row_begin || row_end > h->M) return SEXTANS_ERR_INVALID;
    const bool whole = row_begin == 0 && row_end == h->M;
    const int nrows = row_end - row_begin;
    if (ldb < h->K || ldc < nrows || ldc_in < nrows) return SEXTANS_ERR_INVALID;
    SX_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    // A call without the reuse flag announces a new B: whatever panels the workspace holds are stale from here on,
    // also when THIS call does not repack (column-major staging, fuse_b) -- a later chunk of the same pipelined SpMM
    // that does need panels must not find those of an earlier B.  (An empty range too: the next call, which will carry
    // the flag, must not find the panels of some earlier B.)
    if (!(flags & SEXTANS_ROWS_REUSE_B_PANELS)) h->bp_layout = 0;
    if (nrows == 0) return SEXTANS_OK;
    Tiling t;
    if (int rc = prepare(h, N, whole, &t)) return rc;
    if (h->dense_W > 0) {
        // Dense tiles first, on the matrix cores: C_out = alpha * (A_dense * bf16(B)) + beta * C_in for the full block
        // rows (and alpha * 0 + beta * C_in below them); the CSR kernels then add alpha * (A_rest * B) on top
        // (their beta becomes 1, their C_in the partial result): one C pass per kernel, no extra combine launch.
        if (!whole || (N % 32) != 0) {
            g_last_error = "mfma_dense_tiles = 1 needs whole-matrix calls and N % 32 == 0";
            return SEXTANS_ERR_INVALID;
        }
        if (int rc = launch_dense_tiles(h, N, alpha, d_B, ldb, beta, d_C_in, ldc_in, d_C_out, ldc, s)) return rc;
        beta = 1.0f; d_C_in = d_C_out; ldc_in = ldc;
    }
    const Call c{N, alpha, d_B, ldb, beta, d_C_in, ldc_in, d_C_out, ldc, row_begin, row_end, flags, s, whole};
    const RouteCM r = route_cm(h, c, std::move(t));
    switch (r.path) {
        case RouteCM::kWindow: return run_window(h, c, r);
        case RouteCM::kColwise: return run_colwise(h, c);
        default: return run_segments(h, c, r);
    }
}

}  // extern "C"
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
// row-major rows x cols (ld_rm) <-> column-major (ld_cm); cols % 4 == 0
void launch_transpose_skinny(bool to_cm, const float *src, float *dst, int64_t ld_rm, int64_t ld_cm, int rows, int cols, hipStream_t s) {
    if (rows <= 0 || cols <= 0) return;
    const int cw = cols >= 32 ? 32 : 16;
    const dim3 grid((unsigned)((rows + 63) / 64), (unsigned)((cols + cw - 1) / cw));
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, src, dst, ld_rm, ld_cm, rows, cols); };
    if (cw == 32) { if (to_cm) go(transpose_skinny<true, 32>); else go(transpose_skinny<false, 32>); }
    else { if (to_cm) go(transpose_skinny<true, 16>); else go(transpose_skinny<false, 16>); }
}
void launch_transpose(const float *src, int64_t ld_src, float *dst, int64_t ld_dst, int rows, int cols, hipStream_t s) {
    if (rows <= 0 || cols <= 0) return;
    hipLaunchKernelGGL(transpose_tiles, dim3((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32)), dim3(256), 0, s, src, ld_src, dst, ld_dst, rows, cols);
}
__global__ __launch_bounds__(256) void invert_positions(int K, const int *__restrict__ colpos, int *__restrict__ colinv) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < K) colinv[colpos[k]] = k;
}
__global__ __launch_bounds__(256) void translate_dict(long long n, int K, const int *__restrict__ dict, const int *__restrict__ colinv, int *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) { const int c = dict[i]; out[i] = (unsigned)c < (unsigned)K ? colinv[c] : 0; }   // (slots past a block's dictionary are never used)
}
}  // namespace
extern "C" {

// The order in which the clustered plan visits the rows, for callers that can RENUMBER their matrix once (what FEM packages do with
// RCM): order[i] = row at position i.  A contiguous range of the renumbered matrix is a compact piece of the matrix graph, so the
// row-range partition of sextans_dist_spmm hands every rank a cluster -- its own part of B plus a halo instead of all of B -- and the
// natural-order forms of the renumbered matrix run like the reordered form without its passes.  (A contiguous range of a RANDOMLY
// numbered mesh holds 1 / world of every row's neighbours: 3.3 x compute-phase speed-up at 8 ranks, profiles/r05_rank_slab_times.json.)
// The reference's scheduler likewise fixes the order of the non-zeros once, on the host (sparse_helper.h:345-403).
int sextans_export_row_order(sextans_handle_t h, int *order, int *clustered) {
    if (!h || !order) return SEXTANS_ERR_INVALID;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    SX_HIP(hipSetDevice(h->device));
    if (int rc = prepare(h, 16)) return rc;
    const bool have = h->cluster_state > 0 && h->d_slot_row && h->psc.plan_built && h->nhub == 0 && h->nchain == 0;
    if (clustered) *clustered = have ? h->cluster_state : 0;
    if (!have) {
        for (int i = 0; i < h->M; ++i) order[i] = i;
        return SEXTANS_OK;
    }
    int *d_tab = nullptr;
    SX_HIP(hipMalloc((void **)&d_tab, sizeof(int) * (size_t)std::max(h->M, 1)));
    cc_table(h, 0, d_tab, nullptr);
    const hipError_t e = hipMemcpy(order, d_tab, sizeof(int) * (size_t)h->M, hipMemcpyDeviceToHost);
    (void)hipFree(d_tab);
    SX_HIP(e);
    return SEXTANS_OK;
}

// Row-major operands.  The reference lays B and C out for its kernel on the host, OUTSIDE the timed call (sextans-host.cpp:150-195,
// 264-270); a caller whose operands are row-major (torch tensors; the natural layout of a "K x N feature matrix") gets the same here:
// no layout pass at all on the LDS-panel paths.
}  // extern "C"
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
    if ((h->cluster_state == -1 || h->cluster_runs) && h->cluster_decline == 12 && !h->cluster_rm_tried && t.W == 16 && h->opt_row_cluster < 0) {
        h->cluster_rm_tried = true;
        free_cluster_plan(h);
        h->cluster_for_rm = true;
        const int rc = prepare(h, Nplan, true, &t);
        h->cluster_for_rm = false;
        if (rc) return rc;
    }
    if (t.W == 16 && h->cluster_state == 2 && h->d_colpos && !h->d_dict_nat) {   // the plan's dictionaries hold relabelled columns: translate them back once
        const long long n = (long long)h->psc.plan_nblk * h->psc.plan_dict_stride;
        int *colinv = nullptr;
        if (hipMalloc((void **)&colinv, sizeof(int) * (size_t)std::max(h->K, 1)) != hipSuccess ||
            hipMalloc((void **)&h->d_dict_nat, sizeof(int) * (size_t)std::max<long long>(n, 1)) != hipSuccess) {
            (void)hipFree(colinv); (void)hipFree(h->d_dict_nat); h->d_dict_nat = nullptr; (void)hipGetLastError();
            g_last_error = "row-major plan: out of device memory for the translated block dictionaries";
            return SEXTANS_ERR_HIP;
        }
        hipLaunchKernelGGL(invert_positions, dim3((unsigned)((h->K + 255) / 256)), dim3(256), 0, s, h->K, h->d_colpos, colinv);
        hipLaunchKernelGGL(translate_dict, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, h->K, h->psc.d_dict, colinv, h->d_dict_nat);
        const hipError_t se = hipStreamSynchronize(s);
        (void)hipFree(colinv);
        SX_HIP(se);
    }
    if (out) *out = std::move(t);
    return SEXTANS_OK;
}
}  // namespace sxe
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

}  // extern "C"
namespace {
// Everything sextans_spmm_device_rm decides for one call (route_rm), before anything is launched
struct RouteRM {
    enum Path { kColwise, kPanelV2, kRowgroup, kTranspose } path = kTranspose;
    bool aligned = false;        // 16-byte aligned operands with leading dimensions that are multiples of 4
    int mode = -1;               // kPanelV2: launch_panel_v2's mode -- 0 natural order, 1 grid bricks, 2 graph clustering
    bool split = false;          // kPanelV2 on a mixed plan: dictionary blocks there, the other blocks' rows on the gather kernel
    std::vector<Seg> segs;       // kRowgroup: the tiling of N
};

RouteRM route_rm(const sextans_engine *h, const Call &c, const Tiling &t) {
    RouteRM r;
    const bool colwise = colwise_wanted(h);
    r.aligned = ((reinterpret_cast<uintptr_t>(c.B) | reinterpret_cast<uintptr_t>(c.C_in) | reinterpret_cast<uintptr_t>(c.C_out)) & 15) == 0 &&
                c.ldb % 4 == 0 && c.ldc_in % 4 == 0 && c.ldc % 4 == 0;
    // 32-bit offsets inside the kernel: floats into B (C beyond 4 GB: the kernel's 64-bit form, launch_panel_v2)
    const bool fits = (int64_t)h->K * c.ldb < ((int64_t)1 << 32);
    // Rows on the long-row paths (pieces, exact chains): from the caller's row-major B into its row-major C as well -- the piece kernel's
    // 16-byte gathers and the chain producers' LDS-DMA read B rows ldb floats apart instead of panel rows, the fold and the chain
    // consumer write C[r * ldc + n].  The main kernels skip those rows (d_skip), so the order between the launches does not matter;
    // the chains run beside the main kernel on the engine's side stream, as in the column-major form.
    const bool hubs = h->nhub > 0, chains = h->nchain > 0;
    const bool long_ok = (!hubs && !chains) || (r.aligned && (!chains || (h->aux_stream && h->ev_fork && h->ev_join && c.ldb < ((int64_t)1 << 31))));
    if (colwise && r.aligned && !hubs && !chains && csr_only(h) && h->m_nnz > 0) {   // short rows in a local numbering: lane per row, 16-byte accesses
        r.path = RouteRM::kColwise;
        return r;
    }
    if (t.W == 16 && (h->opt_kernel == 0 || h->opt_kernel == 2) && h->opt_panel_v2 != 0 && h->opt_cols_per_lane != 8 && csr_only(h) &&
        !(colwise && !hubs && !chains) && r.aligned && fits && long_ok && h->m_nnz > 0) {
        if (h->cluster_state == 2) r.mode = 2;
        else if (h->cluster_state == 1) r.mode = 1;
        else if (t.panel && (!h->ps.plan_mixed || (h->ps.d_rg_skip && h->opt_split_mixed != 0 && h->opt_kernel == 0)) && h->ps.plan_max_dict <= sx::kWideMaxDict) r.mode = 0;
    }
    if (r.mode == 2 && h->d_colpos && !h->d_dict_nat) r.mode = -1;   // (cannot happen after rm_plan; kept as a guard)
    if (r.mode >= 0) {
        r.path = RouteRM::kPanelV2;
        r.split = r.mode == 0 && h->ps.plan_mixed;
        return r;
    }
    // The gather kernel on a matrix without rows on the piece / chain / dense-tile paths: a row of row-major B IS what its lanes fetch
    // per non-zero (the 4 * LPR floats of a panel row), and a lane's 4 accumulators are 16 bytes of its C row -- no repack, no passes.
    if (!t.panel && !t.window && !(colwise && !hubs && !chains) && r.aligned && long_ok && (h->opt_kernel == 0 || h->opt_kernel == 1) && csr_only(h) && h->m_nnz > 0) {
        r.path = RouteRM::kRowgroup;
        r.segs = t.segs;
        if (c.N == 8) r.segs.assign(1, Seg{8, 0, 1});   // (the plan above was made for 16 columns)
        return r;
    }
    // Everything else (lane-per-row / window kernels, mixed plans, rows on the piece and chain paths, dense tiles, unaligned operands):
    // through column-major copies in the engine's workspaces
    return r;
}


int run_rm_colwise(sextans_engine *h, const Call &c) {
    Prof p(h, &h->ev_kernel, c.s);
    auto go = [&](auto kern, int col0, int ntiles) {
        // groups of T neighbouring lanes per row, one 16-column tile each (T = the largest divisor of the tile count up to 8): a
        // wavefront's loads cover T * 64 consecutive bytes of every row it touches
        int T = 1;
        if (h->opt_colwise_tiles_adjacent != 0)
            for (int t = 8; t > 1; --t)
                if (ntiles % t == 0) { T = t; break; }
        const int rows_per = sx::kBlock / T, nrowblk = (h->M + rows_per - 1) / rows_per, ygrid = ntiles / T;
        const int adj = T == 1 && ntiles > 1 && h->opt_colwise_tiles_adjacent != 0 && (int64_t)nrowblk * ntiles < ((int64_t)1 << 31) ? ntiles : 0;
        hipLaunchKernelGGL(kern, adj ? dim3((unsigned)nrowblk * (unsigned)ntiles) : dim3((unsigned)nrowblk, (unsigned)ygrid), dim3(sx::kBlock), 0, c.s, h->m_rp, h->m_ci,
                           h->m_v, c.B, c.ldb, c.C_in, c.ldc_in, c.C_out, c.ldc, 0, h->M, nrowblk, col0, c.alpha, c.beta, (int)h->opt_xcd, (const unsigned char *)h->d_skip, adj, T);
    };
    const int n16 = c.N / 16;
    if (n16 > 0) { if (h->opt_exact) go(sx::spmm_csr_colwise<true, 16, true>, 0, n16); else go(sx::spmm_csr_colwise<false, 16, true>, 0, n16); }
    if (c.N % 16) { if (h->opt_exact) go(sx::spmm_csr_colwise<true, 8, true>, n16 * 16, 1); else go(sx::spmm_csr_colwise<false, 8, true>, n16 * 16, 1); }
    h->last_kernel = "spmm_csr_colwise_rowmajor";
    SX_HIP(hipGetLastError());
    return SEXTANS_OK;
}

// The paths on the caller's row-major operands (kPanelV2, kRowgroup), rows on the long-row paths included
int run_rm_direct(sextans_engine *h, const Call &c, const RouteRM &r) {
    Prof p(h, &h->ev_kernel, c.s);
    const bool long_rows = h->nhub > 0 || h->nchain > 0;
    if (h->nchain > 0) {
        std::vector<Seg> segs;   // tiles of the chain kernel: 16-column tiles and an 8-column tail (never past column N of a B row)
        if (c.N / 16) segs.push_back(Seg{16, 0, c.N / 16});
        if (c.N % 16) segs.push_back(Seg{8, c.N / 16 * 16, 1});
        if (int rc = fork_chains(h, c, segs, 0, h->nchain, true)) return rc;
    }
    // the gather kernel: over the rows of the blocks without a dictionary (split form of a mixed plan), or over all rows
    auto rowgroups = [&](const std::vector<Seg> &segs, const unsigned char *skip, const int *groups, int ngroups) {
        for (const Seg &g : segs)
            by_width(g.width, [&](auto L) {
                launch_rowgroup<decltype(L)::value>(h, h->m_rp, h->m_rp + 1, h->m_ci, h->m_v, false, skip, c.B + g.col0, c.C_in + g.col0, c.ldc_in,
                                                    c.C_out + g.col0, c.ldc, 0, h->M, g.ntiles, c.alpha, c.beta, c.s, c.ldb, false, groups, ngroups);
                return SEXTANS_OK;
            });
    };
    if (r.path == RouteRM::kPanelV2) {
        const int ntiles = (c.N + 15) / 16, last_cols = c.N % 16 ? 8 : 16;
        const sextans_engine::PanelState &P = r.mode ? h->psc : h->ps;
        if (int rc = launch_panel_v2<1>(h, c.B, c.C_in, c.ldc_in, c.C_out, c.ldc, ntiles, c.alpha, c.beta, c.s, 0, 0, P.plan_nblk, 0, r.mode, last_cols, c.ldb, r.split))
            return rc;
        if (r.split) rowgroups(wide_first(c.N), h->ps.d_rg_skip, h->ps.d_rg_groups, h->ps.rg_ngroups);
    } else {
        rowgroups(r.segs, h->d_skip, nullptr, 0);
    }
    if (h->nhub > 0) {   // the long rows' pieces and their fold
        const sextans_engine::PieceTable &pt = h->by_len;
        const int v0 = pt.h_vfirst[0], v1 = pt.h_vfirst[(size_t)h->nhub];
        for (const Seg &g : wide_first(c.N))
            by_width(g.width, [&](auto L) {
                launch_hub_pieces<decltype(L)::value>(h, pt, c.B + g.col0, g.ntiles, g.col0, v0, v1, c.s, nullptr, c.ldb);
                return SEXTANS_OK;
            });
        launch_fold(h, pt, 0, h->nhub, c.N, c.C_in, c.ldc_in, c.C_out, c.ldc, 0, c.alpha, c.beta, true, c.s);
    }
    if (h->nchain > 0) SX_HIP(hipStreamWaitEvent(c.s, h->ev_join, 0));
    h->last_kernel = r.path == RouteRM::kRowgroup ? (long_rows ? "spmm_csr_rowgroup_rowmajor+long_rows" : "spmm_csr_rowgroup_rowmajor")
                     : r.mode == 2 ? (long_rows ? "spmm_csr_panel_v2_rowmajor_clustered+long_rows" : "spmm_csr_panel_v2_rowmajor_clustered")
                                   : (long_rows ? "spmm_csr_panel_v2_rowmajor+long_rows" : "spmm_csr_panel_v2_rowmajor");
    SX_HIP(hipGetLastError());
    return SEXTANS_OK;
}

// Column-major copies in the engine's workspaces -- two transposes in front, one behind -- around the column-major entry point.
// (workspaces of their own -- not the host-buffer entry points' d_B / d_Cin / d_Cout, which are filled on another stream; C_in and
// C_out may alias, so one C buffer)
int run_rm_transpose(sextans_engine *h, const Call &c, bool aligned) {
    const int N = c.N;
    h->lean_prepare = false;
    const size_t nB = (size_t)h->K * (size_t)N, nC = (size_t)h->M * (size_t)N;
    if (int rc = ensure(&h->d_rmB, &h->rmB_cap, nB)) return rc;
    if (int rc = ensure(&h->d_rmC, &h->rmC_cap, nC)) return rc;
    {
        Prof p(h, &h->ev_repack, c.s);
        if (aligned) {
            launch_transpose_skinny(true, c.B, h->d_rmB, c.ldb, h->K, h->K, N, c.s);
            launch_transpose_skinny(true, c.C_in, h->d_rmC, c.ldc_in, h->M, h->M, N, c.s);
        } else {
            launch_transpose(c.B, c.ldb, h->d_rmB, h->K, h->K, N, c.s);
            launch_transpose(c.C_in, c.ldc_in, h->d_rmC, h->M, h->M, N, c.s);
        }
    }
    if (int rc = sextans_spmm_device_rows(h, N, c.alpha, h->d_rmB, h->K, c.beta, h->d_rmC, h->M, h->d_rmC, h->M, 0, h->M, 0, (void *)c.s)) return rc;
    {
        Prof p(h, &h->ev_post, c.s);
        if (aligned) launch_transpose_skinny(false, h->d_rmC, c.C_out, c.ldc, h->M, h->M, N, c.s);
        else launch_transpose(h->d_rmC, h->M, c.C_out, c.ldc, N, h->M, c.s);
    }
    SX_HIP(hipGetLastError());
    return SEXTANS_OK;
}
}  // namespace
extern "C" {

int sextans_spmm_device_rm(sextans_handle_t h, int N, float alpha, const float *d_B, int64_t ldb, float beta, const float *d_C_in,
                           int64_t ldc_in, float *d_C_out, int64_t ldc, void *stream) {
    if (!h || N <= 0 || (N % 8) != 0 || !d_B || !d_C_in || !d_C_out || ldb < N || ldc_in < N || ldc < N) return SEXTANS_ERR_INVALID;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    SX_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (h->M == 0) return SEXTANS_OK;
    Tiling t;
    if (int rc = rm_plan(h, N, s, &t)) return rc;
    const Call c{N, alpha, d_B, ldb, beta, d_C_in, ldc_in, d_C_out, ldc, 0, h->M, 0, s, true};
    const RouteRM r = route_rm(h, c, t);
    switch (r.path) {
        case RouteRM::kColwise: return run_rm_colwise(h, c);
        case RouteRM::kTranspose: return run_rm_transpose(h, c, r.aligned);
        default: return run_rm_direct(h, c, r);
    }
}

}  // extern "C"

// ---- bf16 dense operands on the row-major entry (spmm_bf16_kernels.h) --------------------------------------------------------------
namespace sxe {
int check_rm_bf16_args(sextans_handle_t h, int N, const uint16_t *d_B, int64_t ldb, const void *d_C_in, int64_t ldc_in, void *d_C_out,
                       int64_t ldc, int c_dtype) {
    if (!h || N <= 0 || (N % 8) != 0 || !d_B || !d_C_in || !d_C_out || ldb < N || ldc_in < N || ldc < N) return SEXTANS_ERR_INVALID;
    if (c_dtype != SEXTANS_DTYPE_F32 && c_dtype != SEXTANS_DTYPE_BF16) return SEXTANS_ERR_INVALID;
    const uintptr_t cmask = c_dtype == SEXTANS_DTYPE_BF16 ? 1 : 3;   // addresses that cannot hold an element of their type
    if ((reinterpret_cast<uintptr_t>(d_B) & 1) || ((reinterpret_cast<uintptr_t>(d_C_in) | reinterpret_cast<uintptr_t>(d_C_out)) & cmask)) return SEXTANS_ERR_INVALID;
    return SEXTANS_OK;
}
}  // namespace sxe
namespace {
// The bf16 kernels' tiling of N: 64-column tiles (8 lanes per row, a whole 128-byte line of a B row), then at most one 32-, 16- and 8-column tile
std::vector<Seg> bf16_tiles(int N) {
    std::vector<Seg> v;
    int col = 0;
    if (N / 64) { v.push_back(Seg{64, 0, N / 64}); col = N / 64 * 64; }
    for (int w : {32, 16, 8})
        if ((N - col) / w) { v.push_back(Seg{w, col, 1}); col += w; }
    return v;
}
template <class F>
void by_width_bf16(int width, F f) {   // f(LPR): 8 columns per lane
    switch (width) {
        case 64: f(std::integral_constant<int, 8>{}); break;
        case 32: f(std::integral_constant<int, 4>{}); break;
        case 16: f(std::integral_constant<int, 2>{}); break;
        default: f(std::integral_constant<int, 1>{}); break;
    }
}

struct CallBf16 {
    int N; float alpha; const uint16_t *B; int64_t ldb; float beta; const void *C_in; int64_t ldc_in; void *C_out; int64_t ldc; bool cbf16; hipStream_t s;
};

// The native route: the gather kernel (and the piece path of long rows) on the caller's bf16 buffers.  The very arrays run_rm_direct
// passes (m_rp / m_ci / m_v, the piece table by_len) -- what a value refresh rewrites.
int run_rm_bf16_native(sextans_engine *h, const CallBf16 &c) {
    Prof p(h, &h->ev_kernel, c.s);
    const size_t esz = c.cbf16 ? 2 : 4;
    const bool stage = h->opt_stage != 0, exact = h->opt_exact != 0;
    for (const Seg &g : bf16_tiles(c.N))
        by_width_bf16(g.width, [&](auto L) {
            constexpr int LPR = decltype(L)::value, RB = sx::kBlock / LPR, CH = 2048;
            const int nrowblk = (h->M + RB - 1) / RB;
            auto go = [&](auto kern) {
                hipLaunchKernelGGL(kern, dim3((unsigned)nrowblk * (unsigned)g.ntiles), dim3(sx::kBlock), 0, c.s, h->m_rp, h->m_rp + 1, h->m_ci, h->m_v,
                                   c.B + g.col0, c.ldb, (const void *)((const char *)c.C_in + esz * (size_t)g.col0), c.ldc_in,
                                   (void *)((char *)c.C_out + esz * (size_t)g.col0), c.ldc, h->M, g.ntiles, nrowblk, c.alpha, c.beta, (int)h->opt_xcd,
                                   (const unsigned char *)h->d_skip);
            };
#define SX_BF(EX, ST) (c.cbf16 ? go(sx::spmm_csr_rowgroup_bf16<LPR, CH, EX, ST, true>) : go(sx::spmm_csr_rowgroup_bf16<LPR, CH, EX, ST, false>))
            if (exact) { if (stage) SX_BF(true, true); else SX_BF(true, false); }
            else       { if (stage) SX_BF(false, true); else SX_BF(false, false); }
#undef SX_BF
        });
    if (h->nhub > 0) {   // the long rows' pieces (raw fp32 sums into P) and their fold
        const sextans_engine::PieceTable &pt = h->by_len;
        const int v0 = pt.h_vfirst[0], v1 = pt.h_vfirst[(size_t)h->nhub];
        for (const Seg &g : bf16_tiles(c.N))
            by_width_bf16(g.width, [&](auto L) {
                constexpr int LPR = decltype(L)::value, RB = sx::kBlock / LPR;
                const int nblk = (v1 - v0 + RB - 1) / RB;
                if (nblk <= 0) return;
                auto go = [&](auto kern) {
                    hipLaunchKernelGGL(kern, dim3((unsigned)nblk * (unsigned)g.ntiles), dim3(sx::kBlock), 0, c.s, pt.d_vrp, pt.d_vend, h->s_ci, h->s_v,
                                       c.B + g.col0, c.ldb, h->d_P + (int64_t)g.col0 * h->split_nv, (int64_t)h->split_nv, v0, v1, g.ntiles);
                };
                if (exact) go(sx::spmm_csr_pieces_bf16<LPR, true>); else go(sx::spmm_csr_pieces_bf16<LPR, false>);
            });
        if (c.cbf16) {
            const int64_t tot = (int64_t)h->nhub * c.N;
            auto go = [&](auto kern) {
                hipLaunchKernelGGL(kern, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c.s, pt.d_vfirst, pt.d_row, h->d_P, (int64_t)h->split_nv,
                                   (const uint16_t *)c.C_in, c.ldc_in, (uint16_t *)c.C_out, c.ldc, h->nhub, c.N, c.alpha, c.beta);
            };
            if (exact) go(sx::fold_hub_pieces_bf16<true>); else go(sx::fold_hub_pieces_bf16<false>);
        } else {
            launch_fold(h, pt, 0, h->nhub, c.N, (const float *)c.C_in, c.ldc_in, (float *)c.C_out, c.ldc, 0, c.alpha, c.beta, true, c.s);
        }
    }
    h->last_kernel = h->nhub > 0 ? "spmm_csr_rowgroup_rowmajor_bf16+long_rows" : "spmm_csr_rowgroup_rowmajor_bf16";
    SX_HIP(hipGetLastError());
    ++h->bf16_native_calls;
    return SEXTANS_OK;
}

void launch_widen(const uint16_t *src, int64_t lds, float *dst, int64_t ldd, int64_t rows, int cols, hipStream_t s) {
    if (rows <= 0) return;
    const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0 && lds % 8 == 0 && ldd % 4 == 0;
    const int64_t n = vec ? rows * (cols / 8) : rows * cols;
    if (vec) hipLaunchKernelGGL(sx::widen_bf16_matrix<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, lds, dst, ldd, rows, cols);
    else hipLaunchKernelGGL(sx::widen_bf16_matrix<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, lds, dst, ldd, rows, cols);
}
void launch_round(const float *src, int64_t lds, uint16_t *dst, int64_t ldd, int64_t rows, int cols, hipStream_t s) {
    if (rows <= 0) return;
    const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0 && lds % 4 == 0 && ldd % 8 == 0;
    const int64_t n = vec ? rows * (cols / 8) : rows * cols;
    if (vec) hipLaunchKernelGGL(sx::round_bf16_matrix<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, lds, dst, ldd, rows, cols);
    else hipLaunchKernelGGL(sx::round_bf16_matrix<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, lds, dst, ldd, rows, cols);
}

// the converting route's fp32 copies: B always, C only when it is bf16
int ensure_bf16_workspaces(sextans_engine *h, int N, bool cbf16) {
    if (int rc = ensure(&h->d_bfB, &h->bfB_cap, (size_t)h->K * (size_t)N)) return rc;
    if (cbf16)
        if (int rc = ensure(&h->d_bfC, &h->bfC_cap, (size_t)h->M * (size_t)N)) return rc;
    return SEXTANS_OK;
}

// Every other route: fp32 copies of B (and of a bf16 C) in the engine's workspaces around the fp32 row-major entry point
int run_rm_bf16_converted(sextans_engine *h, const CallBf16 &c) {
    if (int rc = ensure_bf16_workspaces(h, c.N, c.cbf16)) return rc;
    {
        Prof p(h, &h->ev_repack, c.s);
        launch_widen(c.B, c.ldb, h->d_bfB, c.N, h->K, c.N, c.s);
        if (c.cbf16) launch_widen((const uint16_t *)c.C_in, c.ldc_in, h->d_bfC, c.N, h->M, c.N, c.s);
    }
    SX_HIP(hipGetLastError());
    if (!c.cbf16) {
        if (int rc = sextans_spmm_device_rm(h, c.N, c.alpha, h->d_bfB, c.N, c.beta, (const float *)c.C_in, c.ldc_in, (float *)c.C_out, c.ldc, (void *)c.s)) return rc;
    } else {
        if (int rc = sextans_spmm_device_rm(h, c.N, c.alpha, h->d_bfB, c.N, c.beta, h->d_bfC, c.N, h->d_bfC, c.N, (void *)c.s)) return rc;
        Prof p(h, &h->ev_post, c.s);
        launch_round(h->d_bfC, c.N, (uint16_t *)c.C_out, c.ldc, h->M, c.N, c.s);
    }
    SX_HIP(hipGetLastError());
    ++h->bf16_converted_calls;
    return SEXTANS_OK;
}

// 16-byte accesses on the caller's buffers: aligned bases, whole 16-byte groups per row; 32-bit byte offsets into B
bool bf16_aligned(const sextans_engine *h, const CallBf16 &c) {
    const int64_t cm = c.cbf16 ? 8 : 4;
    return (int64_t)h->K * c.ldb * 2 < ((int64_t)1 << 32) && ((reinterpret_cast<uintptr_t>(c.B) | reinterpret_cast<uintptr_t>(c.C_in) | reinterpret_cast<uintptr_t>(c.C_out)) & 15) == 0 &&
           c.ldb % 8 == 0 && c.ldc_in % cm == 0 && c.ldc % cm == 0;
}
// route_rm's decision for the call, unchanged: native where it is the gather kernel and no row is an exact chain
// (asked with the caller's leading dimensions; a call that converts asks again inside sextans_spmm_device_rm with ldb = N of the
// workspace -- route_rm looks at ldb only for alignment and the 32-bit limit of the panel paths, so the two cannot disagree on the gather route)
bool bf16_native(const sextans_engine *h, const CallBf16 &c, const Tiling &t) {
    if (!bf16_aligned(h, c) || h->nchain > 0) return false;
    const Call f{c.N, c.alpha, (const float *)c.B, c.ldb, c.beta, (const float *)c.C_in, c.ldc_in, (float *)c.C_out, c.ldc, 0, h->M, 0, c.s, true};
    return route_rm(h, f, t).path == RouteRM::kRowgroup;
}
}  // namespace
extern "C" {

int sextans_spmm_device_rm_bf16(sextans_handle_t h, int N, float alpha, const uint16_t *d_B, int64_t ldb, float beta, const void *d_C_in,
                                int64_t ldc_in, void *d_C_out, int64_t ldc, int c_dtype, void *stream) {
    if (int rc = check_rm_bf16_args(h, N, d_B, ldb, d_C_in, ldc_in, d_C_out, ldc, c_dtype)) return rc;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    SX_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (h->M == 0) return SEXTANS_OK;
    Tiling t;
    if (int rc = rm_plan(h, N, s, &t)) return rc;
    const CallBf16 c{N, alpha, d_B, ldb, beta, d_C_in, ldc_in, d_C_out, ldc, c_dtype == SEXTANS_DTYPE_BF16, s};
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
    const CallBf16 c{N, 1.f, nullptr, N, 0.f, nullptr, N, nullptr, N, c_dtype == SEXTANS_DTYPE_BF16, s};
    if (bf16_native(h, c, t)) return SEXTANS_OK;
    return ensure_bf16_workspaces(h, N, c.cbf16);
}

}  // extern "C"
namespace {
// The timed region of the host-buffer entry points: [pre] + rp_time x SpMM from h->d_B / h->d_Cin into
// h->d_Cout + [post], on the engine's own stream.  B is the same in every repeat, so its panel repack runs
// in the first one only (the reference re-lays B out on the host, outside its timed region:
// sextans-host.cpp:150-177).  The repeats are captured once into a hipGraph (instantiated outside the timed
// region) and replayed with a single launch: the loop is launch-bound for small matrices (nasa4704: 4.3 us
// per repeat replayed vs 7.8 us launched one by one).
template <class Pre, class Post>
int run_repeats(sextans_engine *h, int N, float alpha, float beta, int rp_time, Pre pre, Post post, double *ns) {
    if (!h->host_stream) {
        SX_HIP(hipStreamCreateWithFlags(&h->host_stream, hipStreamNonBlocking));
        // first use of a stream sets up its hardware queue (~1 ms): keep that out of the timed region
        SX_HIP(hipMemsetAsync(h->d_Cout, 0, 4, h->host_stream));
        SX_HIP(hipStreamSynchronize(h->host_stream));
    }
    hipStream_t cs = h->host_stream;
    // `count` repeats; the first one lays B out in panels, the others reuse them.  Loops of four or more
    // repeats always use the panel-staged kernel (one repack amortised) instead of the column-major staging.
    const int nofuse = rp_time >= 4 ? kRowsNoFuseB : 0;
    auto enqueue = [&](int count) -> int {
        for (int r = 0; r < count; ++r)
            if (int rc = sextans_spmm_device_rows(h, N, alpha, h->d_B, h->K, beta, h->d_Cin, h->M, h->d_Cout, h->M,
                                                  0, h->M, (r ? SEXTANS_ROWS_REUSE_B_PANELS : 0) | nofuse, (void *)cs))
                return rc;
        return SEXTANS_OK;
    };
    struct Cleanup {   // released on every exit path
        hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Cleanup() {
            if (exec) (void)hipGraphExecDestroy(exec);
            if (graph) (void)hipGraphDestroy(graph);
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
        }
    } c;
    const int per_graph = rp_time < 128 ? rp_time : 128;   // bound the graph; long loops replay it
    bool use_graph = !h->opt_profile && !h->opt_phase_timing;
    if (use_graph) {
        // relaxed mode: the enqueue path calls hipSetDevice / hipGetLastError, which thread-local capture rejects
        SX_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeRelaxed));
        const int rc = enqueue(per_graph);
        const hipError_t ce = hipStreamEndCapture(cs, &c.graph);
        // A capture can be invalidated from OUTSIDE: any host thread of the process that touches the legacy default stream meanwhile (a
        // plain hipMemcpy in the caller's own code is enough) makes HIP fail it.  The graph is an optimisation of the launch path, not
        // a requirement: without it the repeats are launched one by one -- same kernels, same bits.
        if (rc != SEXTANS_OK || ce != hipSuccess || !c.graph || hipGraphInstantiate(&c.exec, c.graph, nullptr, nullptr, 0) != hipSuccess) {
            if (c.graph) (void)hipGraphDestroy(c.graph);
            c.graph = nullptr; c.exec = nullptr;
            use_graph = false;
            h->graph_fallbacks += 1;
            // (the invalidated capture leaves the stream unusable in this HIP version -- every later launch on it reports "previous error
            // during capture": the repeats run on a fresh stream)
            (void)hipStreamDestroy(h->host_stream);
            h->host_stream = nullptr;
            for (int i = 0; i < 4 && hipGetLastError() != hipSuccess; ++i) {}
            SX_HIP(hipStreamCreateWithFlags(&h->host_stream, hipStreamNonBlocking));
            cs = h->host_stream;
        }
    }
    SX_HIP(hipEventCreate(&c.e0));
    SX_HIP(hipEventCreate(&c.e1));
    SX_HIP(hipEventRecord(c.e0, cs));
    if constexpr (!std::is_same<Pre, std::nullptr_t>::value) pre(cs);
    if (use_graph) {
        for (int done = 0; done + per_graph <= rp_time; done += per_graph) SX_HIP(hipGraphLaunch(c.exec, cs));
        if (int rc = enqueue(rp_time % per_graph)) return rc;
    } else if (int rc = enqueue(rp_time)) {
        return rc;
    }
    if constexpr (!std::is_same<Post, std::nullptr_t>::value) post(cs);
    SX_HIP(hipGetLastError());
    SX_HIP(hipEventRecord(c.e1, cs));
    SX_HIP(hipEventSynchronize(c.e1));
    float ms = 0.f;
    SX_HIP(hipEventElapsedTime(&ms, c.e0, c.e1));
    *ns = (double)ms * 1e6;
    return SEXTANS_OK;
}
}  // namespace
extern "C" {

int sextans_spmm_host(sextans_handle_t h, int N, float alpha, const float *B, float beta, float *C,
                      int rp_time, double *elapsed_ns) {
    if (!h || !B || !C || N <= 0 || (N % 8) != 0) return SEXTANS_ERR_INVALID;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    if (rp_time < 1) rp_time = 1;
    SX_HIP(hipSetDevice(h->device));
    const size_t nB = (size_t)h->K * (size_t)N, nC = (size_t)h->M * (size_t)N;
    if (int rc = ensure(&h->d_B, &h->B_cap, nB)) return rc;
    size_t ccap = h->C_cap;
    if (int rc = ensure(&h->d_Cin, &ccap, nC)) return rc;
    if (int rc = ensure(&h->d_Cout, &h->C_cap, nC)) return rc;
    SX_HIP(hipMemcpy(h->d_B, B, nB * sizeof(float), hipMemcpyHostToDevice));
    SX_HIP(hipMemcpy(h->d_Cin, C, nC * sizeof(float), hipMemcpyHostToDevice));
    if (int rc = prepare(h, N)) return rc;   // allocations and the one-time packing of A stay outside the timed region
    double ns = 0.0;
    if (int rc = run_repeats(h, N, alpha, beta, rp_time, nullptr, nullptr, &ns)) return rc;
    if (elapsed_ns) *elapsed_ns = ns;
    SX_HIP(hipMemcpy(C, h->d_Cout, nC * sizeof(float), hipMemcpyDeviceToHost));
    return SEXTANS_OK;
}

int sextans_set_matrix_edges(sextans_handle_t h, const int32_t *edge_list_ptr, const uint64_t *const *edge_list_ch,
                             int NUM_ITE, int NUM_A_LEN, int M, int K) {
    if (!h || !edge_list_ptr || !edge_list_ch || NUM_ITE < 0 || M < 0 || K < 0) return SEXTANS_ERR_INVALID;
    // NUM_ITE = ceil(K / 4096) (sextans-host.cpp:221): checked BEFORE edge_list_ptr[NUM_ITE] is read
    if ((int64_t)NUM_ITE != ((int64_t)K + SEXTANS_EDGES_WINDOW - 1) / SEXTANS_EDGES_WINDOW) return SEXTANS_ERR_INVALID;
    if (edge_list_ptr[NUM_ITE] != NUM_A_LEN) return SEXTANS_ERR_INVALID;
    int64_t nnz = 0;
    int *rp = nullptr, *ci = nullptr;
    float *v = nullptr;
    if (int rc = sextans_edges_decode_csr(edge_list_ptr, edge_list_ch, NUM_ITE, M, K, &nnz, &rp, &ci, &v))
        return rc;
    const int rc = sextans_set_matrix_csr(h, M, K, nnz, rp, ci, v);
    free(rp); free(ci); free(v);
    return rc;
}

int sextans_invoke(sextans_handle_t h, const int32_t *edge_list_ptr, const uint64_t *const *edge_list_ch,
                   const float *const *mat_B_ch, int num_ch_b, const float *const *mat_C_ch_in,
                   float *const *mat_C_ch, int NUM_ITE, int NUM_A_LEN, int M, int K, int P_N, int alpha_u,
                   int beta_u, double *elapsed_ns) {
    const int N = P_N & 0xFFFF;                      // sextans-host.cpp:223, sextans.cpp:203
    int rp_time = (int)((unsigned)P_N >> 16);
    if (rp_time < 1) rp_time = 1;
    if (!h || !mat_B_ch || !mat_C_ch_in || !mat_C_ch || N <= 0 || (N % 8) || (num_ch_b != 4 && num_ch_b != 8) ||
        M < 0 || K < 0)
        return SEXTANS_ERR_INVALID;
    if (edge_list_ptr) {
        if (int rc = sextans_set_matrix_edges(h, edge_list_ptr, edge_list_ch, NUM_ITE, NUM_A_LEN, M, K)) return rc;
    } else if (!h->d_rp) {
        return SEXTANS_ERR_STATE;
    } else if (h->M != M || h->K != K) {
        return SEXTANS_ERR_INVALID;
    }
    float alpha, beta;
    memcpy(&alpha, &alpha_u, 4);                     // raw fp32 bits, sextans-host.cpp:225-229
    memcpy(&beta, &beta_u, 4);
    SX_HIP(hipSetDevice(h->device));
    const int64_t b_cs = sextans_chan_b_colsize(K, num_ch_b), b_len = sextans_chan_b_len(K, N, num_ch_b);
    const int64_t c_cs = sextans_chan_c_colsize(M), c_len = sextans_chan_c_len(M, N);
    const int64_t b_used = b_cs * (N / 8), c_used = c_cs * (N / 8);
    const size_t nB = (size_t)K * (size_t)N, nC = (size_t)M * (size_t)N;
    if (int rc = ensure(&h->d_chB, &h->chB_cap, (size_t)b_len * num_ch_b)) return rc;
    if (int rc = ensure(&h->d_chC, &h->chC_cap, (size_t)c_len * 8)) return rc;
    if (int rc = ensure(&h->d_B, &h->B_cap, nB)) return rc;
    size_t ccap = h->C_cap;
    if (int rc = ensure(&h->d_Cin, &ccap, nC)) return rc;
    if (int rc = ensure(&h->d_Cout, &h->C_cap, nC)) return rc;
    for (int c = 0; c < num_ch_b; ++c) {
        if (!mat_B_ch[c]) return SEXTANS_ERR_INVALID;
        SX_HIP(hipMemcpy(h->d_chB + (size_t)c * b_len, mat_B_ch[c], sizeof(float) * (size_t)b_used,
                         hipMemcpyHostToDevice));
    }
    for (int c = 0; c < 8; ++c) {
        if (!mat_C_ch_in[c] || !mat_C_ch[c]) return SEXTANS_ERR_INVALID;
        SX_HIP(hipMemcpy(h->d_chC + (size_t)c * c_len, mat_C_ch_in[c], sizeof(float) * (size_t)c_used,
                         hipMemcpyHostToDevice));
    }
    if (int rc = prepare(h, N)) return rc;
    const float pad = alpha * 0.0f + beta * 0.0f;    // what the accelerator writes into rows M .. colsize-1
    auto pre = [&](hipStream_t cs) {
        if (K > 0)
            sx::chan_unpack_b<<<dim3((unsigned)((K + 255) / 256), (unsigned)N), 256, 0, cs>>>(
                h->d_chB, b_len, b_cs, num_ch_b, K, N, h->d_B);
        if (M > 0)
            sx::chan_unpack_c<<<dim3((unsigned)((M + 255) / 256), (unsigned)(N / 8)), 256, 0, cs>>>(
                h->d_chC, c_len, c_cs, M, N, h->d_Cin);
    };
    auto post = [&](hipStream_t cs) {
        if (c_cs > 0)
            sx::chan_pack_c<<<dim3((unsigned)((c_cs + 255) / 256), (unsigned)(N / 8)), 256, 0, cs>>>(
                h->d_Cout, M, N, c_len, c_cs, pad, h->d_chC);
    };
    double ns = 0.0;
    if (M > 0) {
        if (int rc = run_repeats(h, N, alpha, beta, rp_time, pre, post, &ns)) return rc;
    } else {
        pre(nullptr); post(nullptr);
        SX_HIP(hipDeviceSynchronize());
    }
    if (elapsed_ns) *elapsed_ns = ns;
    for (int c = 0; c < 8; ++c)
        SX_HIP(hipMemcpy(mat_C_ch[c], h->d_chC + (size_t)c * c_len, sizeof(float) * (size_t)c_used,
                         hipMemcpyDeviceToHost));
    return SEXTANS_OK;
}

int sextans_spmm_csr(int M, int N, int K, int NNZ, float ALPHA, const int *CSRRowPtr,
                     const int *CSRColIndex, const float *CSRVal, const float *mat_B, float BETA,
                     float *mat_C) {
    sextans_handle_t h = nullptr;
    if (int rc = sextans_create(&h, 0)) return rc;
    int rc = sextans_set_matrix_csr(h, M, K, NNZ, CSRRowPtr, CSRColIndex, CSRVal);
    if (!rc) rc = sextans_spmm_host(h, N, ALPHA, mat_B, BETA, mat_C, 1, nullptr);
    sextans_destroy(h);
    return rc;
}

int sextans_profile_reset(sextans_handle_t h) {
    if (!h) return SEXTANS_ERR_INVALID;
    for (auto *vec : {&h->ev_kernel, &h->ev_repack, &h->ev_post}) {
        for (auto &ep : *vec) { (void)hipEventDestroy(ep.a); (void)hipEventDestroy(ep.b); }
        vec->clear();
    }
    return SEXTANS_OK;
}

int sextans_profile_read(sextans_handle_t h, double *mean_kernel_ns, int64_t *launches,
                         double *mean_repack_ns) {
    if (!h) return SEXTANS_ERR_INVALID;
    SX_HIP(hipSetDevice(h->device));
    auto mean = [&](std::vector<EventPair> &v, double *out) -> int {
        double tot = 0.0;
        for (auto &ep : v) {
            SX_HIP(hipEventSynchronize(ep.b));
            float ms = 0.f;
            SX_HIP(hipEventElapsedTime(&ms, ep.a, ep.b));
            tot += (double)ms * 1e6;
        }
        if (out) *out = v.empty() ? 0.0 : tot / (double)v.size();
        return SEXTANS_OK;
    };
    if (int rc = mean(h->ev_kernel, mean_kernel_ns)) return rc;
    if (int rc = mean(h->ev_repack, mean_repack_ns)) return rc;
    if (launches) *launches = (int64_t)h->ev_kernel.size();
    return SEXTANS_OK;
}

int sextans_profile_read_post(sextans_handle_t h, double *mean_post_ns, int64_t *launches) {
    if (!h) return SEXTANS_ERR_INVALID;
    SX_HIP(hipSetDevice(h->device));
    double tot = 0.0;
    for (auto &ep : h->ev_post) {
        SX_HIP(hipEventSynchronize(ep.b));
        float ms = 0.f;
        SX_HIP(hipEventElapsedTime(&ms, ep.a, ep.b));
        tot += (double)ms * 1e6;
    }
    if (mean_post_ns) *mean_post_ns = h->ev_post.empty() ? 0.0 : tot / (double)h->ev_post.size();
    if (launches) *launches = (int64_t)h->ev_post.size();
    return SEXTANS_OK;
}

const char *sextans_last_kernel(sextans_handle_t h) { return h ? h->last_kernel : "none"; }

int sextans_device_free(int device, void *d_ptr) {
    SX_HIP(hipSetDevice(device));
    SX_HIP(hipFree(d_ptr));
    return SEXTANS_OK;
}

int sextans_device_alloc(int device, size_t bytes, void **d_ptr) {
    if (!d_ptr) return SEXTANS_ERR_INVALID;
    *d_ptr = nullptr;
    SX_HIP(hipSetDevice(device));
    SX_HIP(hipMalloc(d_ptr, std::max<size_t>(bytes, 4)));
    return SEXTANS_OK;
}

int sextans_device_copy(int device, void *dst, const void *src, size_t bytes, int kind) {
    if (kind < SEXTANS_COPY_HOST_TO_DEVICE || kind > SEXTANS_COPY_DEVICE_TO_DEVICE || (bytes && (!dst || !src))) return SEXTANS_ERR_INVALID;
    if (!bytes) return SEXTANS_OK;
    SX_HIP(hipSetDevice(device));
    const hipMemcpyKind k = kind == SEXTANS_COPY_HOST_TO_DEVICE ? hipMemcpyHostToDevice : kind == SEXTANS_COPY_DEVICE_TO_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    SX_HIP(hipMemcpy(dst, src, bytes, k));   // (thread_stream.h: an asynchronous copy on the calling thread's stream + a wait -- never the legacy stream)
    return SEXTANS_OK;
}

}  // extern "C"