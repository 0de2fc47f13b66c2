// engine_launch.h -- every kernel launch of the SpMM paths (engine_launch.hip), behind plain functions: the routes (engine_spmm.hip,
// engine_rowmajor.hip, engine_host.hip, the cc_* chunks of engine_dist.hip) decide, these launch.  engine_launch.hip is the only unit
// that sees the kernel templates; a tile width (`width`: columns per tile) and every option arrive as run-time values and become
// template arguments there (dispatch.h).  Not a public header.
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

// groups: the launch covers only these groups of 128 rows (row_begin must be 0)
// rm_ldb > 0: dBp / dCin / dCout are the caller's ROW-major operands at this segment's first column (sextans_spmm_device_rm)
// round_robin: workgroups to the XCDs in launch order (the split form of a mixed plan: most workgroups leave at once, and contiguous
// chunks per XCD would put all the working ones on one or two XCDs)
void launch_rowgroup(sextans_engine *h, int width, const int *rp, const int *rend, const int *ci, const float *va, bool pieces,
                     const unsigned char *skip, const float *dBp, const float *dCin, int64_t ldc_in, float *dCout, int64_t ldc, int row_begin,
                     int row_end, int ntiles, float alpha, float beta, hipStream_t s, int64_t rm_ldb = 0, bool round_robin = false, const int *groups = nullptr, int ngroups = 0);
// dBp: repacked panel (bcol_ld == 0) or the caller's column-major B at this segment's first column with its
// leading dimension bcol_ld (dictionary-only plans, small B: no repack launch).
int launch_panel(sextans_engine *h, int width, const float *dBp, const float *dCin, int64_t ldc_in, float *dCout, int64_t ldc, int ntiles,
                 float alpha, float beta, hipStream_t s, int64_t bcol_ld, int blk_begin, int blk_end, int row_base);
// Wide-N form of the panel kernel (spmm_panel_v2.h): `nsuper` super tiles of H * 16 columns (H = 1 or 2) starting at the pointers
// given; dictionary-only plans built for 4 lanes per row.  mode, rm_ldb, dict_blocks_only: see the definition.
int launch_panel_v2(sextans_engine *h, int H, const float *dBp, const float *dCin, int64_t ldc_in, float *dCout, int64_t ldc, int nsuper,
                    float alpha, float beta, hipStream_t s, int64_t bcol_ld, int blk_begin, int blk_end, int row_base, int mode = 0,
                    int last_cols = 16, int64_t rm_ldb = 0, bool dict_blocks_only = false);
// dBp8: N/8 row-major K x 8 panels.  Rows [wave_begin * RW, min(M, wave_end * RW)); the C pointers address
// row `row_base` as their row 0.
void launch_window(sextans_engine *h, const float *dBp8, const float *dCin, int64_t ldc_in, float *dCout, int64_t ldc, int ntiles,
                   int wave_begin, int wave_end, int row_base, float alpha, float beta, hipStream_t s);
// The lane-per-row kernel on the caller's own operands, rows [row_begin, row_end): column-major (rm = false) or row-major
void launch_colwise(sextans_engine *h, bool rm, int N, const float *B, int64_t ldb, const float *dCin, int64_t ldc_in, float *dCout,
                    int64_t ldc, int row_begin, int row_end, float alpha, float beta, hipStream_t s);
// Exact chains of the chain rows [c0, c1) (chain_fused, spmm_csr_kernels.h): products from the repacked B panels (segment by
// segment, like the piece kernel) and the serial sum of every (row, column) in one workgroup, epilogue included.
void launch_chains(sextans_engine *h, const std::vector<Seg> &plan, const float *dCin, int64_t ldc_in, float *dCout, int64_t ldc, int N,
                   int c0, int c1, int row_base, float alpha, float beta, hipStream_t s, bool permuted_panels = false, const float *rm_B = nullptr, int64_t rm_ldb = 0);
// Hub rows: pieces [v0, v1) of piece table t summed as virtual rows from B panels of `width` columns at dBp (ntiles panels) into
// h->d_P.  rm_ldb > 0: dBp is the caller's row-major B at column col0 (sextans_spmm_device_rm)
void launch_hub_pieces(sextans_engine *h, int width, const sextans_engine::PieceTable &t, const float *dBp, int ntiles, int col0, int v0,
                       int v1, hipStream_t s, const int *colpos = nullptr, int64_t rm_ldb = 0);
// The partial sums of the long rows [hub0, hub1) of piece table t folded in order into C (rm: the caller's row-major C)
void launch_fold(sextans_engine *h, const sextans_engine::PieceTable &t, int hub0, int hub1, int N, const float *dCin, int64_t ldc_in,
                 float *dCout, int64_t ldc, int row_base, float alpha, float beta, bool rm, hipStream_t s);
// row-major rows x cols (ld_rm) -> column-major (ld_cm), or (to_cm false) back.  aligned: cols % 4 == 0 and the row-major side 16-byte
// aligned with ld_rm % 4 == 0 -- the skinny form in 16-byte accesses; otherwise 32 x 32 tiles
void launch_transpose(bool aligned, bool to_cm, const float *src, float *dst, int64_t ld_rm, int64_t ld_cm, int rows, int cols, hipStream_t s);

// bf16 dense operands on the row-major entry (spmm_bf16_kernels.h), shaped like their fp32 siblings; `width` columns per tile at 8
// columns per lane, all rows of the main matrix, C fp32 or bf16 (cbf16) at its first column of the tile
void launch_rowgroup_bf16(sextans_engine *h, int width, const uint16_t *B, int64_t ldb, const void *dCin, int64_t ldc_in, void *dCout,
                          int64_t ldc, int ntiles, float alpha, float beta, bool cbf16, hipStream_t s);
void launch_hub_pieces_bf16(sextans_engine *h, int width, const sextans_engine::PieceTable &t, const uint16_t *B, int64_t ldb, int ntiles, int col0, int v0, int v1, hipStream_t s);
void launch_fold_bf16(sextans_engine *h, const sextans_engine::PieceTable &t, int N, const uint16_t *dCin, int64_t ldc_in, uint16_t *dCout,
                      int64_t ldc, float alpha, float beta, hipStream_t s);
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
const char *kernel_name(int main, bool hubs, bool dense);             // static strings for sextans_last_kernel
const char *with_rowblocks(sextans_engine *h, const char *name);      // ... the launches of this call + the fp32 matrix-core one

}  // namespace sxe
