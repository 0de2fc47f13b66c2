// engine_launch.h -- every kernel launch of the SpMM paths (engine_launch.hip), behind plain functions: the routes (engine_spmm.hip,
// engine_rowmajor.hip, engine_host.hip, the cc_* chunks of engine_dist.hip) decide, these launch.  engine_launch.hip is the only unit
// that sees the kernel templates; a tile width (`width`: columns per tile) and every option arrive as run-time values and become
// template arguments there (dispatch.h).  The dense operands cross this seam as ONE description (Operands, engine_state.h): pointers,
// leading dimensions, where B lies (BLayout), alpha / beta, stream, first row -- advanced to the launch's first column by Operands::at;
// a launcher adds only what is its own (tiles, a block / row / piece range; launch_panel_v2: the named fields of PanelV2).  Not a public header.
#pragma once
#include "engine_state.h"

namespace sxe {

// what the routes and the readers of a packed plan need to know about the kernels (engine_launch.hip asserts both against the kernel headers)
constexpr int kBlock = 256;         // threads per workgroup of the SpMM kernels
constexpr int kWideMaxDict = 576;   // dictionary capacity spmm_csr_panel_v2 serves (plans at 4 lanes per row)

void preload_device_code();   // sextans_create: loads the code object now instead of inside the first timed launch

// B (column-major, ldb) -> N-tile panels of `width` columns.  ncols < ntiles * width: the last panel is zero-filled past them
void launch_repack(int width, const float *dB, int64_t ldb, float *dBp, int K, int col_base, int ntiles, hipStream_t s, int k_begin = 0,
                   int k_end = -1, int ncols = -1, const unsigned char *touched = nullptr);
// ... -> 16-column panels in the column order of the graph-clustered plan (h->cluster.d_colpos), rows [col_lo, col_hi) of B
void launch_repack_perm(sextans_engine *h, const float *dB, int64_t ldb, float *dBp, int col_base, int ntiles, int ncols, hipStream_t s);
// row-major 16-column tiles ([tile][M][16]) -> column-major C, columns [col0, col0 + ncols)
void launch_tiles_to_colmajor(const float *tiles, float *C, int64_t ldc, int M, int col0, int ntiles, int ncols, hipStream_t s);

inline Operands on_panels(const sextans_engine *h, Operands o) {   // the same call reading the repacked panels in d_Bp
    o.B = h->d_Bp; o.ldb = h->K; o.layout = BLayout::kPanels;
    return o;
}

// The gather kernel on rows [o.row_base, row_end) of the main matrix, B from panels or the caller's row-major B (sextans_spmm_device_rm).
// groups: the launch covers only these groups of 128 rows (o.row_base must be 0)
void launch_rowgroup(sextans_engine *h, int width, const Operands &o, int ntiles, int row_end, const unsigned char *skip,
                     const int *groups = nullptr, int ngroups = 0);
// B from panels, or the caller's column-major B (dictionary-only plans, small B: no repack launch); row blocks [blk_begin, blk_end)
int launch_panel(sextans_engine *h, int width, const Operands &o, int ntiles, int blk_begin, int blk_end);
// Wide-N form of the panel kernel (spmm_panel_v2.h): `nsuper` super tiles of H * 16 columns starting at the pointers given; dictionary-only
// plans built for 4 lanes per row.  Which plan it walks and how it addresses C:
enum class V2Order {
    kNatural,     // the natural-order plan (h->ps); C in place
    kBricks,      // grid bricks: the plan over the rows in brick order, whole-matrix calls only; its slot -> row table addresses C
    kReordered,   // graph clustering, the reordered form: B = permuted panels, C_in == C_out == the row-major staging buffer, ldc_in ==
                  // ldc == floats per tile; the same slot -> row table addresses the staging rows.  On the caller's row-major operands
                  // it reads B through the plan's dictionaries translated back to the caller's column numbers (h->cluster.d_dict_nat)
    kPositions    // clustered-order chunks of sextans_dist_spmm: the graph-clustered plan with C addressed BY POSITION in the clustered
                  // order (no slot -> row table): C_in == C_out == a packed slab [tile][position][16] of the chunk, ldc_in == ldc == floats per tile
};
struct PanelV2 {   // the defaults are the common launch: every block of the natural-order plan, full 16-column tiles
    int H = 1;                        // 16-column tiles per super tile (1 or 2)
    V2Order order = V2Order::kNatural;
    int blk_begin = 0, blk_end = -1;  // row blocks of the plan (-1: to its last)
    int last_cols = 16;               // valid columns of the last tile (8: the merged tail of N = 16 t + 8)
    bool dict_blocks_only = false;    // mixed plan, split form: the launch walks the plan's d_dict_blocks instead of [blk_begin, blk_end)
};
int launch_panel_v2(sextans_engine *h, const Operands &o, int nsuper, const PanelV2 &a = {});
// o.B: N/8 row-major K x 8 panels.  Rows [wave_begin * RW, min(M, wave_end * RW))
void launch_window(sextans_engine *h, const Operands &o, int ntiles, int wave_begin, int wave_end);
// The lane-per-row kernel on the caller's own operands (column- or row-major, all N columns), rows [o.row_base, row_end)
void launch_colwise(sextans_engine *h, const Operands &o, int N, int row_end);
// Exact chains of the chain rows [c0, c1) (chain_fused, spmm_csr_kernels.h): products from the repacked B panels (segment by segment,
// like the piece kernel) or the caller's row-major B, and the serial sum of every (row, column) in one workgroup, epilogue included.
// o: NOT advanced -- the kernel is told each segment's first column
void launch_chains(sextans_engine *h, const std::vector<Seg> &plan, const Operands &o, int c0, int c1, bool permuted_panels = false);
// Hub rows: pieces [v0, v1) of piece table t summed as virtual rows from `ntiles` tiles of `width` columns of o.B (panels, or the
// caller's row-major B; at column col0) into h->d_P
void launch_hub_pieces(sextans_engine *h, int width, const sextans_engine::PieceTable &t, const Operands &o, int ntiles, int col0, int v0,
                       int v1, const int *colpos = nullptr);
// The partial sums of the long rows [hub0, hub1) of piece table t folded in order into C (all N columns)
void launch_fold(sextans_engine *h, const sextans_engine::PieceTable &t, int hub0, int hub1, int N, const Operands &o);
// row-major rows x cols (ld_rm) -> column-major (ld_cm), or (to_cm false) back.  aligned: cols % 4 == 0 and the row-major side 16-byte
// aligned with ld_rm % 4 == 0 -- the skinny form in 16-byte accesses; otherwise 32 x 32 tiles
void launch_transpose(bool aligned, bool to_cm, const float *src, float *dst, int64_t ld_rm, int64_t ld_cm, int rows, int cols, hipStream_t s);

// bf16 dense operands on the row-major entry (spmm_bf16_kernels.h), shaped like their fp32 siblings; `width` columns per tile at 8
// columns per lane, all rows of the main matrix, C fp32 or bf16 (o.c_elem)
void launch_rowgroup_bf16(sextans_engine *h, int width, const OperandsBf16 &o, int ntiles);
void launch_hub_pieces_bf16(sextans_engine *h, int width, const sextans_engine::PieceTable &t, const OperandsBf16 &o, int ntiles, int col0, int v0, int v1);
void launch_fold_bf16(sextans_engine *h, const sextans_engine::PieceTable &t, int N, const OperandsBf16 &o);   // bf16 C (fp32 C: launch_fold)
void launch_widen(const uint16_t *src, int64_t lds, float *dst, int64_t ldd, int64_t rows, int cols, hipStream_t s);   // bf16 -> fp32
void launch_round(const float *src, int64_t lds, uint16_t *dst, int64_t ldd, int64_t rows, int cols, hipStream_t s);   // fp32 -> bf16

// the accelerator's channel layouts (sextans_invoke, chan_kernels.h)
void launch_chan_unpack_b(const float *ch, int64_t chan_len, int64_t colsize, int num_ch_b, int K, int N, float *B, hipStream_t s);
void launch_chan_unpack_c(const float *ch, int64_t chan_len, int64_t colsize, int M, int N, float *C, hipStream_t s);
void launch_chan_pack_c(const float *C, int M, int N, int64_t chan_len, int64_t colsize, float pad, float *ch, hipStream_t s);

// Rows of 16 floats between row-major tiles and a packed slab through a row table (clustered-order chunks, engine_dist.hip), `ntiles`
// tiles: slab[t][i] = tiles[t][rows[i] - sub], or (scatter) the other way
void launch_slab_rows(bool scatter, float *tiles, int64_t tile_stride, const int *rows, int sub, int n, float *slab, int64_t slab_stride, int ntiles, hipStream_t s);

// N as tiles of `widest` columns, then at most one tile of each narrower width down to 8.  fp32 launches on the caller's row-major B:
// widest = 32, whole 128-byte lines of a B row (4 columns per lane); the bf16 kernels: 64, the same line at 8 columns per lane
std::vector<Seg> widest_first(int N, int widest);
inline std::vector<Seg> wide_first(int N) { return widest_first(N, 32); }
inline std::vector<Seg> bf16_tiles(int N) { return widest_first(N, 64); }
enum class MainKernel { kRowgroup, kPanel, kWindow, kPanelV2 };
const char *kernel_name(MainKernel main, bool hubs, bool dense);      // static strings for sextans_last_kernel
const char *with_rowblocks(sextans_engine *h, const char *name);      // ... the launches of this call + the fp32 matrix-core one

}  // namespace sxe
