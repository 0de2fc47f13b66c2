// engine_spmm.hip -- the column-major SpMM entry (sextans_spmm_device[2|_rows]): what one call runs on is decided first (route_cm,
// choose_launches), then launched path by path (run_window / run_colwise / run_segments) through the launch layer (engine_launch.h).
#include <algorithm>

#include "engine_launch.h"

using namespace sxe;

namespace sxe {
// The chains need one or two wavefronts for about a millisecond: on their own stream, beside the main kernel (fork after the B
// panels are in place, join before the call's work on o.s is considered complete).
int fork_chains(sextans_engine *h, const Operands &o, const std::vector<Seg> &segs, int ch0, int ch1) {
    SX_HIP(hipEventRecord(h->ev_fork, o.s));
    SX_HIP(hipStreamWaitEvent(h->aux_stream, h->ev_fork, 0));
    Operands aux = o;
    aux.s = h->aux_stream;
    launch_chains(h, segs, aux, ch0, ch1);
    SX_HIP(hipEventRecord(h->ev_join, h->aux_stream));
    return SEXTANS_OK;
}
}  // namespace sxe

namespace {
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
    const bool window = t.window && c.row_begin % h->win.rw == 0 && (c.row_end % h->win.rw == 0 || c.row_end == h->M);
    // long rows of this range: entries [hub0, hub1) of a piece table, pieces [v0, v1).  Whole-matrix calls walk the
    // table sorted by length (workgroups of equally long pieces), row ranges the one sorted by row.
    r.pt = c.whole ? &h->split.by_len : &h->split.by_row;
    if (h->split.nhub > 0) {
        const auto &rows = r.pt->h_row;
        if (c.whole) { r.hub1 = h->split.nhub; }
        else {
            r.hub0 = (int)(std::lower_bound(rows.begin(), rows.end(), c.row_begin) - rows.begin());
            r.hub1 = (int)(std::lower_bound(rows.begin(), rows.end(), c.row_end) - rows.begin());
        }
        r.v0 = r.pt->h_vfirst[(size_t)r.hub0]; r.v1 = r.pt->h_vfirst[(size_t)r.hub1];
    }
    r.hubs = r.hub1 > r.hub0;
    r.ch1 = h->split.nchain;
    if (h->split.nchain > 0 && !c.whole) {
        r.ch0 = (int)(std::lower_bound(h->split.h_chain_row.begin(), h->split.h_chain_row.end(), c.row_begin) - h->split.h_chain_row.begin());
        r.ch1 = (int)(std::lower_bound(h->split.h_chain_row.begin(), h->split.h_chain_row.end(), c.row_end) - h->split.h_chain_row.begin());
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
    r.fuse_b = r.panel && !h->ps.plan_mixed && h->opt_fuse_b && !(c.flags & kRowsNoFuseB) && t.segs.size() == 1 && h->dense.rb_n == 0 &&   // (routed row blocks read the repacked panels)
               t.segs[0].width == t.W && !r.hubs && !r.chains &&
               (size_t)h->K * (size_t)N * sizeof(float) <= ((size_t)16 << 20) &&
               // (a graph-clustered plan beats the natural-order blocks of a renumbered matrix also while B fits the L2s, once the
               // matrix is large enough for three more launches not to matter: 332 K rows 123 -> 85 us per step)
               // (... and below that size once the call is large enough: a 13 965-row matrix in a random node order, N = 128,
               // 112 us staged from column-major B on its natural-order plan against 34 us reordered; N = 16: 13.3 against 15.0.
               // Crossover measured at ~24 M non-zero x column products: tools/small_renumbered.py)
               !(c.whole && h->cluster.state == 2 && h->cluster.cm_pays && (h->M >= 65536 || h->m_nnz * (int64_t)N >= ((int64_t)24 << 20)));
    // (Staging from column-major B for LARGE matrices -- no repack launch at all -- was measured in round 4 and loses everywhere: 4M-row
    // 3-dof FEM N = 16 kernel 660 -> 872 us against 83 us of repack saved; 1-dof 27-point 379 -> 577; 2-D 9-point 296 -> 427;
    // 5-point 270 -> 412: 36 four-byte loads per lane and panel through registers instead of nine LDS-DMA requests.)
    // The reordered form (graph-clustered plan, ensure_cluster_plan): whole-matrix calls, 16-column tiles.  Its B panels hold the
    // rows of B in the plan's column order and C goes through the block-major staging buffer (reorder_kernels.h); an 8-column
    // remainder tile keeps the natural-order kernels and panels.  (Layout tag -W: such panels are never reused by a row-range call.)
    r.reordered = c.whole && h->cluster.state == 2 && h->cluster.cm_pays && h->opt_kernel != 1 && h->opt_kernel != 3 && t.W == 16 && !r.fuse_b &&
                  (!r.chains || h->cluster.d_chain_ci_perm) && csr_only(h) && h->d_Cs &&
                  // (the staging buffer is sized by prepare() for the N it saw: a plan that survived a set_option("kernel") and a
                  // larger N since then must not run past its end -- ADVICE r04)
                  h->d_Cs.size() >= (size_t)((N + 15) / 16) * (size_t)h->M * 16 && (N >= 16 || (N == 8 && !r.hubs && !r.chains));
    r.cs_tile = r.reordered ? (int64_t)h->M * 16 : 0;
    // 32-bit byte offsets inside the wide kernels: panels and C columns (wide_fits), and the caller's B when the kernel stages
    // from it (wide_fits_b)
    const bool wide_fits = h->ps.plan_max_dict <= kWideMaxDict && (int64_t)h->K * 64 < ((int64_t)1 << 32) &&
                           std::max(c.o.ldc, c.o.ldc_in) * 64 < ((int64_t)1 << 32);
    const bool wide_fits_b = wide_fits && (!r.fuse_b || c.o.ldb * 64 < ((int64_t)1 << 32));
    // N = 16 t + 8 on the register-resident panel kernel: the 8-column tail used to go to the gather kernel (the plan is built for
    // 16-column tiles) -- 4M-row FEM matrix: N = 24 2 152 us per step against 1 099 at N = 32.  It now runs as one more 16-column tile:
    // its B panel is zero in the 8 columns that do not exist, the kernel neither loads nor stores C there (`last_cols`), the passes of
    // the reordered form skip them; rows on the piece path sum 16 columns into their (wider) partial-sum buffer and fold N, the exact
    // chains take the tail as one 8-column tile of the 16-column panel.  Not with dense tiles on the MFMA path or column-major staging.
    const bool v2 = r.reordered || (r.panel && !h->ps.plan_mixed && h->opt_panel_v2 != 0 && !r.fuse_b && wide_fits && h->opt_cols_per_lane != 8);
    std::vector<Seg> &plan = r.segs;
    plan = std::move(t.segs);
    if (v2 && t.W == 16 && plan.size() == 2 && plan[0].width == 16 && plan[1].width == 8 && plan[1].ntiles == 1 &&
        (h->split.nhub == 0 || h->d_P.size() >= (size_t)h->split.nv * (size_t)(N + 8)) &&
        // (with rows on the piece / chain paths only where the main rows are long enough to matter: on the KKT class -- 6 entries per
        // row, arrow borders as chains -- the wider piece / chain work cost more than the gather tail: 1 510 -> 1 687 us at N = 24)
        ((h->split.nhub == 0 && h->split.nchain == 0) || (h->M > 0 && h->m_nnz / h->M >= 16)) &&
        csr_only(h) && h->d_Bp.size() >= (size_t)h->K * (size_t)(N + 8) &&
        (!r.reordered || h->d_Cs.size() >= (size_t)(N / 16 + 1) * (size_t)h->M * 16)) {
        plan[0].ntiles += 1;
        plan[0].last_cols = 8;
        plan.pop_back();
    } else if (v2 && t.W == 16 && plan.size() == 1 && plan[0].width == 8 && plan[0].ntiles == 1 && h->split.nhub == 0 && h->split.nchain == 0 &&
               csr_only(h) && h->d_Bp.size() >= (size_t)h->K * 16 && (!r.reordered || h->d_Cs.size() >= (size_t)h->M * 16)) {
        plan[0] = Seg{16, 0, 1, 8};   // N = 8 on the 16-column plan (engine_plan.hip: prepare, n8_wide)
    }
    r.layout = r.reordered ? -t.W : plan[0].last_cols != 0 ? t.W + 100 : t.W;
    r.skip_repack = r.fuse_b || ((c.flags & SEXTANS_ROWS_REUSE_B_PANELS) != 0 && h->bp_layout == r.layout);
    // whole-matrix calls on repacked panels: the plan over the rows in clustered (brick) order when the matrix has one
    r.clustered = c.whole && !r.fuse_b && h->cluster.state == 1;
    choose_launches(h, c, t.W, wide_fits_b, r);
    return r;
}

int run_window(sextans_engine *h, const Call &c, const RouteCM &r) {
    const int N = c.N;
    hipStream_t s = c.o.s;
    // B in 8-column panels (the reference's N tile), then one tile-major launch
    if (!r.skip_repack) {
        Prof p(h, &h->ev_repack, s);
        launch_repack(8, c.o.B, c.o.ldb, h->d_Bp, h->K, 0, N / 8, s, h->col_lo, h->col_hi, -1, h->mat.d_touched);
        h->bp_layout = r.layout;
    }
    {
        Prof p(h, &h->ev_kernel, s);
        const Operands o = on_panels(h, c.o);
        const int w0 = c.row_begin / h->win.rw, w1 = (c.row_end + h->win.rw - 1) / h->win.rw;
        launch_window(h, o, N / 8, w0, w1);
        const std::vector<Seg> p8{{8, 0, N / 8}};
        if (r.hubs) {
            launch_hub_pieces(h, 8, *r.pt, o, N / 8, 0, r.v0, r.v1);
            launch_fold(h, *r.pt, r.hub0, r.hub1, N, o);
        }
        if (r.chains) launch_chains(h, p8, o, r.ch0, r.ch1);
        h->last_kernel = kernel_name(MainKernel::kWindow, r.hubs || r.chains, h->dense.W > 0);
        if (h->dense.rb_n > 0) {
            // (the row-block kernel takes a 16-column tile from ONE panel: 8-column panels go to it one at a time.  As one segment, the way
            // this call was written before, columns 8 .. 15 of every tile were summed from column 0's B and stored)
            std::vector<Seg> each;
            for (int t = 0; t < N / 8; ++t) each.push_back(Seg{8, 8 * t, 1});
            if (int rc = launch_rowblocks(h, each, o, N, c.row_end)) return rc;
            h->last_kernel = with_rowblocks(h, h->last_kernel);
        }
    }
    SX_HIP(hipGetLastError());
    return SEXTANS_OK;
}

int run_colwise(sextans_engine *h, const Call &c) {
    Prof p(h, &h->ev_kernel, c.o.s);
    launch_colwise(h, c.o, c.N, c.row_end);
    h->last_kernel = "spmm_csr_colwise";
    SX_HIP(hipGetLastError());
    return SEXTANS_OK;
}

// One segment's main launch(es) and, for rows on the piece path, its piece launch
int launch_segment(sextans_engine *h, const Call &c, const RouteCM &r, const Seg &g, RouteCM::Launch l) {
    const Operands panels = on_panels(h, c.o).at(g.col0);       // the segment on the repacked panels
    const Operands src = r.fuse_b ? c.o.at(g.col0) : panels;    // ... or staged from the caller's column-major B
    const int *colpos = nullptr;   // of the piece launch at the end
    PanelV2 a;
    a.blk_begin = r.blk0; a.blk_end = r.blk1;
    switch (l) {
        case RouteCM::kReorderedV2: {
            Operands staged = panels;   // C: the row-major staging buffer, every block of the clustered plan
            staged.C_in = staged.C_out = h->d_Cs; staged.ldc_in = staged.ldc = r.cs_tile; staged.row_base = 0;
            a = PanelV2{};
            a.order = V2Order::kReordered;
            if (int rc = launch_panel_v2(h, staged, g.ntiles, a))
                return rc;   // (a merged tail tile needs no mask here: its staging columns exist, the pass below writes back the valid ones)
            // rows on the piece path: their partial sums from the PERMUTED panels (column c sits at row colpos[c]); folded into C
            // behind the staging -> C pass below, which leaves C_in in their rows
            colpos = h->cluster.d_colpos;
            break;
        }
        case RouteCM::kV2Wide: {
            const int nsuper = g.ntiles / 2;
            a.H = 2;
            if (int rc = launch_panel_v2(h, src, nsuper, a)) return rc;
            if (g.ntiles & 1)   // the odd 16-column tile behind the super tiles
                if (int rc = launch_panel(h, 16, src.at(nsuper * 32), 1, r.blk0, r.blk1)) return rc;
            break;
        }
        case RouteCM::kSplitMixed:
            a.dict_blocks_only = true;
            if (int rc = launch_panel_v2(h, src, g.ntiles, a)) return rc;
            launch_rowgroup(h, 16, panels, g.ntiles, c.row_end, h->ps.d_rg_skip, h->ps.d_rg_groups, h->ps.rg_ngroups);
            break;
        case RouteCM::kV2:
            if (r.clustered) { a = PanelV2{}; a.order = V2Order::kBricks; }
            if (g.last_cols) a.last_cols = g.last_cols;
            if (int rc = launch_panel_v2(h, src, g.ntiles, a)) return rc;
            break;
        case RouteCM::kPanel:
            if (int rc = launch_panel(h, g.width, src, g.ntiles, r.blk0, r.blk1)) return rc;
            break;
        case RouteCM::kRowgroup:
            launch_rowgroup(h, g.width, panels, g.ntiles, c.row_end, h->split.d_skip);
    }
    if (r.hubs) launch_hub_pieces(h, g.width, *r.pt, panels, g.ntiles, g.col0, r.v0, r.v1, colpos);   // (every spmm_csr_panel_v2 segment is 16 columns wide)
    return SEXTANS_OK;
}

int run_segments(sextans_engine *h, const Call &c, const RouteCM &r) {
    const int N = c.N;
    hipStream_t s = c.o.s;
    const Operands panels = on_panels(h, c.o);
    if (!r.skip_repack || r.reordered) {
        Prof p(h, &h->ev_repack, s);
        if (!r.skip_repack) {
            h->bp_layout = r.layout;
            for (const Seg &g : r.segs) {
                float *dst = h->d_Bp + (size_t)h->K * (size_t)g.col0;
                if (r.reordered && g.width == 16 && h->cluster.d_colpos) launch_repack_perm(h, c.o.B, c.o.ldb, dst, g.col0, g.ntiles, g.cols(), s);
                else launch_repack(g.width, c.o.B, c.o.ldb, dst, h->K, g.col0, g.ntiles, s, h->col_lo, h->col_hi, g.cols(), h->mat.d_touched);
            }
        }
        if (r.reordered)
            for (const Seg &g : r.segs)
                if (g.width == 16)
                    launch_repack(16, c.o.C_in, c.o.ldc_in, h->d_Cs, h->M, g.col0, g.ntiles, s, 0, -1, g.cols());   // C_in -> row-major tiles
    }
    {
        Prof p(h, &h->ev_kernel, s);
        if (r.chains && !r.reordered)
            if (int rc = fork_chains(h, panels, r.segs, r.ch0, r.ch1)) return rc;
        for (size_t i = 0; i < r.segs.size(); ++i)
            if (int rc = launch_segment(h, c, r, r.segs[i], r.launch[i])) return rc;
        if (r.hubs && !r.reordered) launch_fold(h, *r.pt, r.hub0, r.hub1, N, panels);
        if (r.chains && !r.reordered) SX_HIP(hipStreamWaitEvent(s, h->ev_join, 0));
        const bool v2_used = std::any_of(r.launch, r.launch + r.segs.size(), [](RouteCM::Launch l) { return l < RouteCM::kPanel; });
        h->last_kernel = r.reordered ? "spmm_csr_panel_v2_reordered"
                                     : kernel_name(v2_used ? MainKernel::kPanelV2 : r.panel ? MainKernel::kPanel : MainKernel::kRowgroup, r.hubs || r.chains, h->dense.W > 0);
        if (h->dense.rb_n > 0) {   // dense blocks of 16 rows on the fp32 matrix cores, from the same panels (the kernels above skipped their rows)
            if (int rc = launch_rowblocks(h, r.segs, panels, N, c.row_end)) return rc;
            h->last_kernel = with_rowblocks(h, h->last_kernel);
        }
    }
    if (r.reordered) {
        Prof p(h, &h->ev_post, s);
        for (const Seg &g : r.segs)
            if (g.width == 16)
                launch_tiles_to_colmajor(h->d_Cs, c.o.C_out, c.o.ldc, h->M, g.col0, g.ntiles, g.cols(), s);
        if (r.hubs) launch_fold(h, *r.pt, r.hub0, r.hub1, N, panels);
        // chain rows write C themselves: behind the staging -> C pass (which left C_in in their rows), from the permuted panels
        if (r.chains) launch_chains(h, r.segs, panels, r.ch0, r.ch1, true);
    }
    SX_HIP(hipGetLastError());
    return SEXTANS_OK;
}
}  // namespace

extern "C" {

int sextans_spmm_device(sextans_handle_t h, int N, float alpha, const float *d_B, int64_t ldb, float beta, const float *d_C_in, float *d_C_out, int64_t ldc, void *stream) {
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
    if (t.window) *aligned = row / h->win.rw * h->win.rw;
    else if (t.panel && !h->ps.h_blk_row.empty())
        *aligned = *(std::upper_bound(h->ps.h_blk_row.begin(), h->ps.h_blk_row.end(), row) - 1);
    return SEXTANS_OK;
}

int sextans_spmm_device2(sextans_handle_t h, int N, float alpha, const float *d_B, int64_t ldb,
                         float beta, const float *d_C_in, int64_t ldc_in, float *d_C_out, int64_t ldc, void *stream) {
    if (!h) return SEXTANS_ERR_INVALID;
    return sextans_spmm_device_rows(h, N, alpha, d_B, ldb, beta, d_C_in, ldc_in, d_C_out, ldc, 0, h->M, 0, stream);
}

int sextans_spmm_device_rows(sextans_handle_t h, int N, float alpha, const float *d_B, int64_t ldb,
                             float beta, const float *d_C_in, int64_t ldc_in, float *d_C_out, int64_t ldc, int row_begin, int row_end, int flags, void *stream) {
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
    Call c;
    c.N = N; c.row_begin = row_begin; c.row_end = row_end; c.flags = flags; c.whole = whole;
    c.o.B = d_B; c.o.ldb = ldb;   // (column-major: OperandsT's defaults)
    c.o.C_in = d_C_in; c.o.ldc_in = ldc_in; c.o.C_out = d_C_out; c.o.ldc = ldc;
    c.o.alpha = alpha; c.o.beta = beta; c.o.s = s; c.o.row_base = row_begin;
    if (h->dense.W > 0) {
        // Dense tiles first, on the matrix cores: C_out = alpha * (A_dense * bf16(B)) + beta * C_in for the full block
        // rows (and alpha * 0 + beta * C_in below them); the CSR kernels then add alpha * (A_rest * B) on top
        // (their beta becomes 1, their C_in the partial result): one C pass per kernel, no extra combine launch.
        if (!whole || (N % 32) != 0) {
            g_last_error = "mfma_dense_tiles = 1 needs whole-matrix calls and N % 32 == 0";
            return SEXTANS_ERR_INVALID;
        }
        if (int rc = launch_dense_tiles(h, N, c.o)) return rc;
        c.o.beta = 1.0f; c.o.C_in = d_C_out; c.o.ldc_in = ldc;
    }
    const RouteCM r = route_cm(h, c, std::move(t));
    switch (r.path) {
        case RouteCM::kWindow: return run_window(h, c, r);
        case RouteCM::kColwise: return run_colwise(h, c);
        default: return run_segments(h, c, r);
    }
}

}  // extern "C"
