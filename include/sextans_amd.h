/*
 * sextans_amd.h -- C ABI of the MI355X-native SpMM engine (drop-in boundary for the Sextans path).
 *
 * Plain C types only: pointers, sizes, scalars.  No torch / C++ types cross this boundary.
 * Every entry point names the reference interface it replaces (paths relative to
 * linghaosong/Sextans, branch tapa).  All functions return 0 (SEXTANS_OK) on success or a
 * SEXTANS_ERR_* code; nothing here ever calls exit() (the reference's loader does,
 * sparse_helper.h:100-109,120-123,146-149,181-191).
 *
 * Conventions shared with the reference:
 *   - A is M x K sparse, B is K x N dense, C is M x N dense, C = alpha*A*B + beta*C
 *     (sparse_helper.h:273-277);
 *   - dense matrices are COLUMN MAJOR fp32 (B[k + ldb*n], C[m + ldc*n]);
 *   - indices are 0-based 32-bit ints, values fp32;
 *   - N is used as given by the caller; the CLI rounds it up to a multiple of 8 first
 *     (sextans-host.cpp:51) via sextans_round_up_n().
 *
 * The compute entry points run ONLY on an AMD GPU (gfx950).  There is no CPU fallback: without
 * a usable HIP device they return SEXTANS_ERR_NO_DEVICE.
 */
#ifndef SEXTANS_AMD_H
#define SEXTANS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ error codes */
#define SEXTANS_OK 0
#define SEXTANS_ERR_OPEN 1         /* "Could not open ..."                  sparse_helper.h:181-184 */
#define SEXTANS_ERR_BANNER 2       /* "Could not process Matrix Market banner" sparse_helper.h:100-103 */
#define SEXTANS_ERR_SIZE 3         /* "Could not read Matrix Market format"  sparse_helper.h:105-109 */
#define SEXTANS_ERR_NOT_COORD 4    /* "... is not a coordinate file!"        sparse_helper.h:188-191 */
#define SEXTANS_ERR_COMPLEX 5      /* "complex matrix, not supported yet!"   sparse_helper.h:120-123 */
#define SEXTANS_ERR_INDEX 6        /* index < 1 (reference) or > M/K (ours)  sparse_helper.h:146-149 */
#define SEXTANS_ERR_ALLOC 7
#define SEXTANS_ERR_PARSE 8        /* malformed entry (the reference reads garbage silently) */
#define SEXTANS_ERR_INVALID 9      /* bad argument */
#define SEXTANS_ERR_NO_DEVICE 10   /* no HIP device / wrong architecture: NO CPU fallback */
#define SEXTANS_ERR_HIP 11         /* a HIP runtime call failed; see sextans_last_error() */
#define SEXTANS_ERR_STATE 12       /* e.g. spmm before set_matrix */
#define SEXTANS_ERR_PEER 13        /* a collective preparation failed on ANOTHER rank (sextans_dist_prepare); this rank's own work was fine */

#define SEXTANS_FMT_CSR 0          /* enum MATRIX_FORMAT {CSR, CSC}, sparse_helper.h:20 */
#define SEXTANS_FMT_CSC 1

const char *sextans_error_string(int code);
/* Thread-local text of the last HIP failure (empty string if none). */
const char *sextans_last_error(void);

/* ------------------------------------------------------------------ L2: host sparse library */

/* Replaces read_suitsparse_matrix (sparse_helper.h:169-259): loads a SuiteSparse Matrix-Market
 * coordinate file into CSR (ptr has M+1 entries, idx = columns) or CSC (ptr has K+1 entries,
 * idx = rows).  Same observable semantics: case-insensitive banner, real/integer/pattern,
 * pattern -> 1.0f, entries whose fp32 bits are exactly 0 are dropped (-0.0 is kept), only
 * `symmetric` mirrors off-diagonals, duplicates kept in file order, nnz is the post-drop
 * post-mirror count.  Output arrays are malloc'ed; release with sextans_host_free(). */
int sextans_mtx_read(const char *path, int format, int *M, int *K, int *nnz, int **ptr, int **idx,
                     float **val);
void sextans_host_free(void *p);

/* Loader throughput.  sextans_mtx_read parses with all host cores (env
 * SEXTANS_LOADER_THREADS overrides).  The binary container holds exactly the arrays it returns:
 *   64-byte header "SXTCSR01", int32 format, M, K, nnz, int64 src_size, src_mtime_ns, 24 reserved bytes;
 *   ptr[(format == CSR ? M : K) + 1], idx[nnz], val[nnz]  (little endian).
 * sextans_mtx_read_cached reads `path` through the container `cache_path` (NULL: path + ".csr.sxbin" /
 * ".csc.sxbin"): a container written for the same format from a source file of the same size and
 * mtime is loaded instead of parsing (*cache_hit = 1); otherwise the text is parsed and the container
 * (re)written, best effort.  Results are identical either way. */
int sextans_matrix_save(const char *path, int format, int M, int K, int nnz, const int *ptr, const int *idx,
                        const float *val);
int sextans_matrix_load(const char *path, int *format, int *M, int *K, int *nnz, int **ptr, int **idx,
                        float **val);
int sextans_mtx_read_cached(const char *path, const char *cache_path, int format, int *M, int *K, int *nnz,
                            int **ptr, int **idx, float **val, int *cache_hit);

/* Matrix-Market `real general` writer (tools: holdout matrices written to disk for the CLI); %.9g keeps every fp32 value. */
int sextans_mtx_write(const char *path, int M, int K, const int *row_ptr, const int *col_idx, const float *val);

/* Replaces CSC_2_CSR (sparse_helper.h:475-509).  Caller provides row_ptr[M+1], col_idx[nnz],
 * csr_val[nnz].  Per-row column order = CSC traversal order (ascending columns). */
int sextans_csc_to_csr(int M, int K, int nnz, const int *col_ptr, const int *row_idx,
                       const float *csc_val, int *row_ptr, int *col_idx, float *csr_val);

/* Replaces the dense-operand initialisation of sextans-host.cpp:94-111:
 * B[k + K*n] = 1.0f;  C[m + M*n] = (float)(1.0*(m+1)*(n+1)/M/N). */
void sextans_init_dense_B(int K, int N, float *B);
void sextans_init_dense_C(int M, int N, float *C);

/* tapa::round_up<8>(N), sextans-host.cpp:51. */
int sextans_round_up_n(int N);

/* Replaces the verification loop of sextans-host.cpp:262-289.  Returns the mismatch count
 * (|a-b| / (min(|a|,|b|) + 1e-4) > 1e-4) and writes the percentage; pass iff *percent < 2.0. */
int sextans_verify(int M, int N, const float *c_cpu, const float *c_dev, float *percent);

/* Throughput formula of sextans-host.cpp:219,255-260: 2*N*(nnz+M)/1e9/seconds. */
double sextans_gflops(int M, int N, int64_t nnz, double seconds);

/* Host golden used ONLY by the CLI's built-in self check (the reference's main() runs
 * cpu_spmm_CSR for the same purpose, sextans-host.cpp:206-219).  It is never a fallback for
 * the device path. */
int sextans_selfcheck_golden(int M, int N, int K, float alpha, const int *row_ptr,
                             const int *col_idx, const float *val, const float *B, float beta,
                             float *C_inout);

/* ------------------------------------------------------------------ packed row-bucketed form of A
 *
 * The engine's counterpart of the reference's packed non-zero stream (generate_edge_list_for_all_PEs
 * + edge_list_64bit, sparse_helper.h:292-473; 64-bit words with a window-local 14-bit column): rows
 * bucketed into blocks of <= 256/lanes_per_row rows whose distinct columns fit the 36 KiB LDS panel;
 * per block an ascending dictionary; per non-zero a 16-bit dictionary index (or the 32-bit column in
 * blocks without reuse) + fp32 value, every row starting on a 4-entry boundary.  sextans_set_matrix_*
 * builds the same arrays internally; these entry points expose them (inspection, tests, reuse). */
typedef struct sextans_packed {
    int M, K;
    int64_t nnz;
    int lanes_per_row;            /* 2, 4 or 8 (N tile = 4 * lanes) */
    int nblk;                     /* row blocks */
    int *blk_row;                 /* nblk + 1: block b owns rows [blk_row[b], blk_row[b+1]) */
    int *dict_ptr;                /* nblk + 1 offsets into dict; empty range = "direct" block */
    int *dict;                    /* distinct columns of each dictionary block, ascending */
    int *row_off;                 /* M + 1: first stream entry of each row (multiple of 4) */
    uint16_t *idx16;              /* stream_len: dictionary index per entry (dictionary blocks); 0xFFFF in the
                                     padding of those rows, whose value is -0.0f: the kernel multiplies such an
                                     entry with a +1.0f row, and x + (-0.0f) == x bit for bit */
    int *col32;                   /* stream_len: column per entry (direct blocks) */
    float *val;                   /* stream_len: value per entry (+-0 in padding) */
    int64_t stream_len;
    int max_dict;                 /* largest dictionary */
    int64_t nnz_in_panel_blocks;  /* non-zeros covered by dictionary blocks */
} sextans_packed;

/* min_reuse_x100: a block gets a dictionary only if nnz >= min_reuse_x100/100 * distinct columns. */
int sextans_pack_csr(int M, int K, const int *row_ptr, const int *col_idx, const float *val,
                     int lanes_per_row, int min_reuse_x100, sextans_packed *out);
void sextans_packed_free(sextans_packed *p);
/* Decoder: reconstructs col_idx[nnz], val[nnz] of the CSR matrix with row extents row_ptr. */
int sextans_unpack_csr(const sextans_packed *p, const int *row_ptr, int *col_idx, float *val);

/* K-windowed stream of A for the accumulator-resident kernel ("kernel" = 3; the reference's own dataflow:
 * B window on chip, partial sums resident, non-zeros pre-bucketed per (PE, window) -- sextans.cpp:337,353-381,
 * 462-570; sparse_helper.h:345-403).  Wavefront g owns rows [g*rows_per_wave, (g+1)*rows_per_wave); its
 * stream is steps [wave_step0[g], wave_step0[g+1]) of 32 entries each (a multiple of 24 steps), ordered by
 * (K window, rank of the entry inside its (row, window), row) so that a row's entries keep their CSR order;
 * no step holds a row twice; padding entries carry the local row `rows_per_wave` (a dummy accumulator).
 * Entry (little endian 64 bit): low word = fp32 value bits, high word = local_row << 23 | column.
 * K must be <= 2^23, rows_per_wave <= 510.  The arrays are what sextans_set_matrix_* builds internally. */
typedef struct sextans_window_packed {
    int M, K;
    int64_t nnz;
    int rows_per_wave, window_cols, nwaves;
    int64_t steps;                /* total steps (stream holds steps * 32 entries + a zero tail of 32 steps) */
    int64_t padded_lower_bound;   /* the dispatcher's cheap estimate of steps * 32 */
    int *wave_step0;              /* nwaves + 1 */
    uint64_t *stream;
} sextans_window_packed;
int sextans_window_pack_csr(int M, int K, const int *row_ptr, const int *col_idx, const float *val,
                            int rows_per_wave, int window_cols, sextans_window_packed *out);
void sextans_window_packed_free(sextans_window_packed *p);

/* ------------------------------------------------------------------ the accelerator's own buffer formats
 *
 * Writer / reader for exactly the buffers the reference host prepares for tapa::invoke(Sextans, ...)
 * (sextans-host.cpp:114-204), so inputs prepared for the FPGA can be consumed by this engine
 * (sextans_invoke below) and results produced in the FPGA's C layout.
 *
 *   A: scheduled non-zero stream of 64 PEs (row % 64) in 4096-column windows, 10-slot spacing between
 *      entries of one row inside a window, bubble padding to the window's longest PE list
 *      (generate_edge_list_for_all_PEs, sparse_helper.h:292-403); packed as 64-bit words
 *      col14<<50 | row18<<32 | fp32 in 8 channels, PE p at channel p%8, slot bitrev3(p/8) of each
 *      8-word group (edge_list_64bit, sparse_helper.h:406-473); bubble = 0x3FFFF<<32 (any word with
 *      row bit 17 set is skipped, sextans.cpp:407).  edge_list_ptr[w+1] = stream length after window w.
 *   B: NUM_CH_B (4 in sextans.h:8, or 8) float channels, sextans-host.cpp:152-177.
 *   C: 8 float channels, row m in channel m%8 at colsize*(n/8) + (m/8)*8 + n%8, colsize = round_up(M,16)
 *      (sextans-host.cpp:179-195 for C_in, :264-270 for C_out). */
#define SEXTANS_EDGES_NUM_PE 64
#define SEXTANS_EDGES_NUM_CH 8
#define SEXTANS_EDGES_WINDOW 4096

typedef struct sextans_edges {
    int32_t M, K;
    int32_t num_windows;          /* NUM_ITE   = ceil(K / 4096)               sextans-host.cpp:221 */
    int32_t num_a_len;            /* NUM_A_LEN = edge_list_ptr[num_windows]   sextans-host.cpp:222 */
    int64_t nnz;                  /* non-bubble words */
    int64_t ptr_len;              /* ints in edge_list_ptr, zero padded to a multiple of 1024 (:131-134) */
    int64_t chan_len;             /* words per channel: round_up(8 * num_a_len, 512) (sparse_helper.h:412-413) */
    int32_t *edge_list_ptr;
    uint64_t *channel[SEXTANS_EDGES_NUM_CH];
} sextans_edges;

/* Writer: CSC (what the reference host feeds its scheduler) -> stream.  M must be <= 64 * 2^17. */
int sextans_edges_pack_csc(int M, int K, int nnz, const int *col_ptr, const int *row_idx, const float *val,
                           sextans_edges *out);
void sextans_edges_free(sextans_edges *e);
/* Reader: stream -> CSR with each row's entries in stream order (the order the accelerator accumulates
 * them in; ascending columns for streams written from a CSC matrix).  Arrays are malloc'ed
 * (sextans_host_free).  SEXTANS_ERR_INDEX if a word addresses a row >= M or a column >= K. */
int sextans_edges_decode_csr(const int32_t *edge_list_ptr, const uint64_t *const *channel, int num_windows,
                             int M, int K, int64_t *nnz, int **row_ptr, int **col_idx, float **val);
/* Container file (little endian): "SXTEDGE1", M, K, num_windows, num_a_len (int32), nnz, ptr_len,
 * chan_len (int64), edge_list_ptr[ptr_len], channel[8][chan_len]. */
int sextans_edges_save(const char *path, const sextans_edges *e);
int sextans_edges_load(const char *path, sextans_edges *out);

/* Dense channel layouts (host side).  N must be a multiple of 8; num_ch_b is 4 or 8.  *_len = floats
 * per channel (padded to 1024 as the reference allocates them); pack writes only the addressed
 * positions (callers zero the buffers first, as the reference does). */
int64_t sextans_chan_b_colsize(int K, int num_ch_b);
int64_t sextans_chan_b_len(int K, int N, int num_ch_b);
int64_t sextans_chan_c_colsize(int M);
int64_t sextans_chan_c_len(int M, int N);
int sextans_chan_pack_b(int K, int N, int num_ch_b, const float *B, float *const *channel);
int sextans_chan_unpack_b(int K, int N, int num_ch_b, const float *const *channel, float *B);
int sextans_chan_pack_c(int M, int N, const float *C, float *const *channel);
int sextans_chan_unpack_c(int M, int N, const float *const *channel, float *C);

/* ------------------------------------------------------------------ L1: the SpMM engine (HIP) */

typedef struct sextans_engine *sextans_handle_t;

/* Number of usable gfx950 devices (0 and SEXTANS_ERR_NO_DEVICE when there is none). */
int sextans_device_count(int *count);

/* Engine bound to one HIP device.  Re-entrant per handle; a handle must not be used from two
 * threads at once (the reference is single-threaded). */
int sextans_create(sextans_handle_t *h, int device);
int sextans_destroy(sextans_handle_t h);

/* Tunables.  key: "kernel" (0 auto, 1 row-group gather, 2 LDS panel, 3 K-windowed accumulator-resident
 * sweep), "window_rows" (rows per wavefront of kernel 3, default 319), "window_cols" (columns per K window,
 * default 65536), "window_unroll" (4 or 8 steps in flight), "window_auto" (1: kernel 0 may choose kernel 3 from
 * its fabric-traffic model; default 0 because the sweep never beat the gather kernel on MI355X),
 * "lanes_per_row" (2/4/8, N-tile = 4*lanes; 0 = auto, the default: 4 for the panel kernel, 8 for the gather
 * kernel when N >= 32), "stage_a" (0/1 stage the CSR stream through LDS), "xcd_remap" (0/1), "exact" (1 = no FMA, reference rounding; 0 = allow FMA), "profile" (0/1 hipEvent
 * per-kernel timing), "phase_timing" (0/1, see sextans_phase_timing_read), "bucket_rows" / "split_rows" (long
 * rows, the load-balancing the reference gets from dealing rows to PEs by row % 64: rows longer than L0 =
 * "bucket_rows" leave the main kernel and are processed in a second launch in order of length, still summed in
 * CSR order = bit-identical; rows longer than T = "split_rows" are cut into pieces of T entries that are summed in
 * parallel and folded in order -- THOSE rows are re-associated and meet the stated 1e-4 tolerance instead of bit
 * identity; sextans_reassociated_rows lists them.  Values: > 0 explicit, 0 off, -1 chosen from the matrix:
 * L0 = max(32, 2 * mean row length), T = max(1024, nnz / 16384).  Defaults: "bucket_rows" = -1 (exact, so it costs
 * nothing in parity), "split_rows" = 0 -- EVERY row is summed in strict CSR order and the result is bit-identical to
 * cpu_spmm_CSR unless the caller opts into re-association with "split_rows" = -1 or > 0 (power-law inputs with rows of
 * 10^5 entries may want that).  "exact_chain" (default 1): in strict-order mode a row longer than max(1024, nnz/16384)
 * is summed by the exact-chain kernel -- producer wavefronts form all rounded products of the row, ONE serial chain of
 * rounded adds per output column consumes them, bit-identical to cpu_spmm_CSR; 0 = such rows stay on the piece
 * kernel (the same bits, ~20x slower for a 400 000-entry row).  Matrices without long rows take none of this path.  "global_nnz": non-zeros of the WHOLE matrix when this engine holds a row range of it (multi-GPU);
 * the automatic T is derived from it so that every rank cuts hub rows exactly as one GPU would; sextans_dist_spmm sets
 * it from an exchanged sum; 0 = this engine's matrix is the whole matrix),
 * "fuse_b" (1 = the panel kernel may stage B straight from column-major B when B is <= 16 MiB and every row block has a dictionary, saving the
 * repack launch; default 1), "panel_min_reuse_x100" (a row block uses the LDS panel when
 * nnz >= value/100 * distinct columns; default 200; decides for N <= 16) and "panel_min_reuse_wide_x100" (the same for
 * N >= 32, default 150: with more columns per B row the panel pays earlier; the packed plan is built once, for the lower
 * of the two), "panel_v2" (-1 auto / 0 / 1: the register-resident form of the panel
 * kernel, spmm_csr_panel_v2), "tiles_per_wg" (N tiles one workgroup of that kernel walks; 0 = auto),
 * "row_cluster" (-1 auto / 0 never / 1 whenever a clustered plan can be built / 2 graph clustering also for grids): the plan of
 *   spmm_csr_panel_v2 may visit the rows in a clustered order on whole-matrix calls -- the rows of a matrix are independent, so
 *   every sum keeps its order and the result stays bit-identical to cpu_spmm_CSR.  Two forms: (1) matrices with Cartesian-grid
 *   stencil structure in natural ordering are visited brick by brick (csrc/row_cluster.hip; stats "grid_stride_line",
 *   "grid_stride_plane"); (2) matrices whose numbering has no locality but whose graph has (meshes in an arbitrary node order) are
 *   aggregated over the matrix graph on the device (csrc/graph_cluster.hip), their columns relabelled in first-touch order, and the
 *   SpMM runs in its REORDERED form: B repacked into permuted panels, C staged block-major (two extra passes over C inside the call;
 *   sextans_last_kernel = "spmm_csr_panel_v2_reordered").  Any M x K since round 5 ("row_similarity"); rows on the long-row paths (pieces, exact chains) are fine.  Stats: "row_cluster"
 *   (1 grid bricks / 2 graph clustering in use, -1 declined, 0 not evaluated yet -- it is evaluated by the first whole-matrix
 *   SpMM with N >= 16), "panel_rows_natural", "panel_rows_clustered" (B rows copied into LDS per 16-column tile), "panel_blocks",
 *   "panel_blocks_clustered", "cluster_shared_fraction" (sampled pre-test of form 2).  The same reason the reference schedules its
 *   non-zeros: keeping the on-chip B window hot (sparse_helper.h:345-403).
 *   Tunables of the two forms (defaults are the measured best; every setting is bit-identical): "small_panel" (1: clustered plans
 *   of short-row matrices are packed for a 320-row panel when every dictionary fits), "row_sets" (2: short-row 3-D grid matrices --
 *   every row <= 32 entries -- use 128-row bricks as two 64-slot row sets on one panel; 3 = 2-D grids too; 1 = never; stat
 *   "row_sets"), "refine_sweeps" (8) / "refine_rows" (62): block refinement of the graph-clustered order, "relabel_columns" (1),
 *   "cluster_top" (depth of the merge tree).
 * "run_cluster" (default 0 = off; 1 = when it copies >= 10 % fewer panel rows; 2 = always): run-level clustering -- matrices in a
 *   numbering WITH locality whose natural row blocks are cut short by the panel capacity and whose graph-clustered plan is not worth
 *   the reordered form's passes ("cluster_decline" 12) keep runs of 16 consecutive rows together and build each row block from up to 4
 *   runs chosen over the graph of runs (no staging, natural B panels; stat "cluster_runs").  Built and measured in round 5: 11.6 % fewer
 *   panel rows on the holdout class, kernel 687 -> 706 us (the C accesses become 64-byte runs, neighbouring blocks stop sharing B lines
 *   in L2): OFF by default, kept as a tested negative result.
 * "row_similarity" (-1 auto / 0 never / 1 always): which graph form (2) clusters the rows over.  A square matrix with a symmetric
 *   pattern is its own graph (column c = row c).  RECTANGULAR matrices have no such reading: their rows are joined to the 16 rows that share the most columns with them
 *   (found through the transposed pattern, csrc/graph_cluster.hip: row_similarity_graph_device) -- the reference schedules any
 *   M x K matrix for its on-chip window too (sparse_helper.h:345-403).  A square matrix with an unsymmetric pattern (sampled: stat
 *   "pattern_symmetry" < 0.98) is clustered over A + A^T -- the pairwise matching needs symmetric weights.  Stat
 *   "cluster_graph_kind": 0 the matrix itself, 1 a row slab's own square pattern ("row_offset"), 2 row similarity, 3 A + A^T.
 * "row_offset" (default -1): the matrix of this engine is the row slab [row_offset, row_offset + M) of a K x K matrix (what a rank of
 *   sextans_dist_spmm holds, which sets it): the graph clustering of "row_cluster" then runs on the slab's own square pattern.
 * "share_index" (default 1): consecutive rows of a block whose 16-bit index lists are equal up to a constant shift keep one copy
 *   of the list (stats "index_stream_entries", "value_stream_entries"); the exported plan carries every row's own list.
 * "colwise_max_len" (default 6; "kernel" = 4 forces it): rows of at most this mean length in a numbering with locality (stat
 *   "row_coherence" >= 0.7) run on the lane-per-row kernel over the caller's column-major operands (no B repack; stat "colwise").
 * "split_mixed" (default 1; 0 = one launch of spmm_csr_panel<MIXED>): a MIXED plan -- some row blocks reuse B rows and have a dictionary,
 *   others (rows with uniformly random columns) do not -- runs in two launches: the blocks with a dictionary on spmm_csr_panel_v2, the
 *   rows of the others on the gather kernel; both walk compact lists.  Whole-matrix calls, column-major and row-major operands (the
 *   latter without copies).  Whole-matrix calls take the split form from 15 % of the non-zeros in blocks with reuse on (the gather
 *   kernel alone below that; every other use of the LDS-panel plan keeps its 50 % threshold).  Stat "mixed_plan": 0 no / 1 mixed, one
 *   launch / 2 mixed, split form.  Bit-identical either way.
 * "colwise_tiles_adjacent" (default 1; 0 = the tile as the slow grid axis, 2 = neighbours at every N): where the lane-per-row kernel puts
 *   the 16-column tiles of a row at N >= 32.  Row-major operands: groups of T lanes per row take neighbouring tiles, so a wavefront's
 *   loads cover whole 128-byte lines (0.25 -> 0.51 of the roofline at N = 32 .. 256); column-major: the two tiles of N = 32 are
 *   neighbours in the launch order (the row block's CSR entries come from HBM once).  Bit-identical either way.
 * "cluster_group" (default 6), "cluster_shape" (0 = default bricks): layout tunables of form (1); measurement switches (below).
 * "small_v2" (default 1: small matrices staged from column-major B size the launch's dictionary capacity and register-resident
 * batches from the plan; 0 = the full-capacity form, for measurements),
 * "cols_per_lane" (0/4 = 16-column tiles at 4 workgroups per CU, the default; 8 = 32-column super tiles at 2 per CU),
 * "bell_shared" (blocked-ELL, N = 256: -1 = use the union-walk kernel spmm_bell_mfma_shared when 8 consecutive block rows
 * share block columns, stat "bell_share" >= 1.5; 0 never; 1 whenever the unions fit), "bell_debug" (measurements only:
 * ablation bits of that kernel, results are wrong when non-zero).  Unknown keys -> SEXTANS_ERR_INVALID.
 * MEASUREMENT SWITCHES -- "bell_debug", "cluster_shape", "cluster_group", "phase_timing", "reordered_xcd", "dist_broadcast_runs", "rowblock_tiles" -- are not part of the drop-in surface:
 * setting one to anything but its default returns SEXTANS_ERR_INVALID unless the process runs with SEXTANS_DEBUG_OPTIONS=1 in
 * its environment (tools/ do; "bell_debug" corrupts C on purpose). */
/* "mfma_dense_tiles" / "dense_tile_fill_x100": north_star's "MFMA only where a tile is actually dense".  The engine
 * always counts the 32x32 tiles of A whose fill reaches dense_tile_fill_x100 % (default 50) -- sextans_get_stat
 * "dense_tiles", "dense_tile_fraction" (share of the non-zeros in such tiles; estimated from a sample of up to 512
 * block rows while mfma_dense_tiles = 0, exact once the tiles are extracted).  With mfma_dense_tiles = 1 the caller
 * opts into bf16 for them: those tiles (values rounded to bf16) times bf16(B) run on v_mfma_f32_32x32x16_bf16 with
 * fp32 accumulation, the rest of A stays on the fp32 CSR kernels, whose epilogue adds the two parts; results then
 * meet the blocked-ELL tolerance (tests/test_dense_tiles_gpu.py), not bit identity.  Needs N % 32 == 0 and
 * whole-matrix calls.  Default 0: fp32 everywhere, bit-identical to cpu_spmm_CSR.
 * mfma_dense_tiles = 2 (round 6): NO precision trade -- dense blocks of 16 consecutive rows run on the FP32 matrix cores
 * (v_mfma_f32_16x16x4_f32, csrc/rowblock_mfma_kernel.h; the reference's PEs multiply and accumulate in fp32 too, sextans.cpp:285-295,
 * 425-446).  A block is routed when its rows are strictly ascending in their columns and its fill = entries / (64 x the groups of 4
 * consecutive columns it touches) reaches dense_tile_fill_x100 %; routed rows are summed ONLY there, walked in ascending column order,
 * and since the instruction is a k-ordered chain of fused multiply-adds the result is BIT-IDENTICAL to the "exact" = 0 kernels
 * (acc = fmaf(a, b, acc), epilogue fmaf(alpha, acc, beta * c)) -- i.e. inside |d| <= 1e-4 * (|alpha| sum|a b| + |beta c|) of
 * cpu_spmm_CSR -- for finite B (a padding zero times an infinite B entry would be NaN where the CSR kernels see no entry at all).  Any N
 * (multiple of 8), whole-matrix and row-range calls, every rank of the multi-GPU forms; "dense_tiles" / "dense_tile_fraction" then
 * count the routed blocks / the share of the non-zeros in them.  MEASURED (round 6, profiles/r06_rowblock_mfma.jsonl): on a
 * block-tridiagonal matrix of fully dense 32 x 32 blocks the path runs the step at 0.75 / 0.43 / 0.35 / 0.30 of the HBM roofline at
 * N = 16 / 64 / 128 / 256 against 0.79 / 0.47 / 0.38 / 0.32 of the VALU kernels with "exact" = 0 (the matrix cores are ~40 % busy, the
 * loop waits for memory and for issue slots in equal parts, and the matrix is within 1.4 x of its memory bound anyway), and FEM
 * matrices fill their fragments to 0.34 (3 dof) - 0.52 (6 dof) only, so two to three times as many multiply-adds are issued as the
 * matrix holds: 1.5 - 2.7 x slower there.  An option for experiments, not a default.
 * Use it with "exact" = 0 so that routed and unrouted rows follow one rounding rule. */
/* ACCURACY MODES (round 6) -- one documented switch instead of three options:
 *   sextans_set_option(h, "mode", SEXTANS_MODE_STRICT)  default.  "exact" = 1, "split_rows" = 0, "mfma_dense_tiles" = 0: every product
 *       rounded, every row summed in CSR order: BIT-IDENTICAL to cpu_spmm_CSR (sparse_helper.h:262-290), stronger than the reference's
 *       own pass criterion.
 *   sextans_set_option(h, "mode", SEXTANS_MODE_FAST)    "exact" = 0 (fused multiply-adds), "split_rows" = -1 (hub rows above
 *       max(1024, nnz / 16384) entries are cut into pieces summed in parallel and folded in order); "mfma_dense_tiles" stays 0 (its
 *       fp32 form, 2, is bit-identical to this mode and may be added by hand; measured, it does not pay yet).  GUARANTEE, per output element:
 *           |C_fast - C_ref| <= 1e-4 * (|alpha| * sum_j |a_ij * b_jn| + |beta * c_in|)
 *       (the condition-aware form of north_star's "within 1e-4 relative error"; the reference's own check is a tolerance
 *       too, sextans-host.cpp:272-282).  Measured distance is ~1e-7 of that scale: fp32 roundoff of a different, but still fp32,
 *       summation.  Deterministic: the same call gives the same bits every time, on every rank count.
 * sextans_get_option(h, "mode", &v): SEXTANS_MODE_STRICT / SEXTANS_MODE_FAST when the three options stand as that mode set them,
 * -1 when they were set apart by hand. */
#define SEXTANS_MODE_STRICT 0
#define SEXTANS_MODE_FAST 1
int sextans_set_option(sextans_handle_t h, const char *key, int64_t value);
int sextans_get_option(sextans_handle_t h, const char *key, int64_t *value);
/* Rows of the current matrix whose sums are re-associated under the current "split_rows" setting (ascending);
 * writes at most `capacity` of them, *count = how many there are.  sextans_get_stat: "reassociated_rows",
 * "split_threshold". */
int sextans_reassociated_rows(sextans_handle_t h, int *rows, int capacity, int *count);
/* The packed row-bucketed form the ENGINE built for the current matrix at `lanes_per_row` (on the device since round 3:
 * the CSR arrays never leave HBM, csrc/plan_device.hip), read back in the public layout of sextans_pack_csr -- the host
 * builder of the same format; the two are byte-identical (tests/test_plan_device_gpu.py).  Free with
 * sextans_packed_free.  Analogue being replaced: generate_edge_list_for_all_PEs + edge_list_64bit on the host,
 * sparse_helper.h:345-473, sextans-host.cpp:114-148. */
int sextans_export_plan(sextans_handle_t h, int lanes_per_row, struct sextans_packed *out);
/* The order in which the clustered plan ("row_cluster") visits the rows of the current matrix: order[i] = row at position i (M ints,
 * host); *clustered (optional) = 0 none (order = identity) / 1 grid bricks / 2 graph clustering.  For callers that can renumber their
 * matrix once -- P A P^T with new_of_old[order[i]] = i, what FEM packages do with RCM: contiguous row ranges of the renumbered matrix are
 * compact pieces of the matrix graph, which is what the row-range partition of sextans_dist_spmm needs on a mesh whose numbering has
 * no locality.  The reference fixes the order of its non-zeros once on the host as well (sparse_helper.h:345-403). */
int sextans_export_row_order(sextans_handle_t h, int *order, int *clustered);
/* Read-only figures about the matrix currently set.  key: "plan_build_s" (seconds spent so far
 * building packed forms of A -- on the device for the panel plan, on the host for the window stream; outside every timed
 * region like the reference's scheduling/packing, sextans-host.cpp:114-148), "window_padded_entries",
 * "window_state" (0 not evaluated, 1 built, -1 rejected), "panel_fraction", "panel_blocks", "piece_path_rows",
 * "reassociated_rows", "bucket_threshold", "split_threshold", "dense_tiles", "dense_tile_fraction",
 * "dense_tiles_on_mfma", "bell_share", "bell_variant" (the matrix-core kernel that the last blocked-ELL call, or the last dense-tile
 * launch of a CSR call with "mfma_dense_tiles" = 1, ran: 1 / 2 / 4 = spmm_bell_mfma<NSUB>, 8 = spmm_bell_mfma_n256, 9 =
 * spmm_bell_mfma_shared, 0 = none so far; sextans_last_kernel names only the family), "row_cluster" and the other clustering figures listed with that option, "device_bytes" (bytes of
 * device memory the engine has asked the runtime for and holds right now: matrix copies, packed plans, tables, workspaces), "col_range_lo" / "col_range_hi" (the rows
 * of B the matrix has columns in: only those are repacked -- a rank of a row-partitioned SpMM over a banded matrix touches
 * 1 / world of B plus a halo), "cluster_decline" (why the graph clustering was not used: 1 not square and "row_similarity" = 0, 2 long-row paths,
 * 3 offsets, 4 natural blocks full, 5 no shared neighbourhoods, 6..9 a builder failed, 10..12 plan unusable / no gain,
 * 13 short rows in a local numbering), "transpose_build_s" (seconds spent building A^T and the plans of its companion engine,
 * sextans_spmm_t_device_rm), "value_refreshes" / "value_refresh_rebuilt" (sextans_update_values*). */
int sextans_get_stat(sextans_handle_t h, const char *key, double *value);

/* Upload a CSR matrix (host pointers) once; later spmm calls reuse the device copy.  This is
 * the analogue of the reference's FPGA-side preparation (generate_edge_list_for_all_PEs +
 * edge_list_64bit, sextans-host.cpp:114-148), which is likewise outside its timed region. */
int sextans_set_matrix_csr(sextans_handle_t h, int M, int K, int64_t nnz, const int *row_ptr,
                           const int *col_idx, const float *val);
/* Same, for arrays that already live on the engine's device (not copied, not owned). */
int sextans_set_matrix_csr_device(sextans_handle_t h, int M, int K, int64_t nnz,
                                  const int *d_row_ptr, const int *d_col_idx, const float *d_val);

/* Replaces tapa::invoke(Sextans, ...) (sextans-host.cpp:237-251, prototype sextans.h:20-26) with
 * the argument meaning of cpu_spmm_CSR (sparse_helper.h:262-272): host buffers in, C updated in
 * place, column major, ld = K for B and M for C.  The kernel runs rp_time (>=1) times, every
 * repeat from the same C input (the reference reads C_in and writes a separate C_out), and
 * *elapsed_ns receives the device time of ALL repeats (tapa::invoke returns the same;
 * sextans-host.cpp:252 divides by rp_time).  Host<->device copies are outside *elapsed_ns.  B is laid
 * out in panels once (first repeat); the repeats are replayed as one hipGraph. */
int sextans_spmm_host(sextans_handle_t h, int N, float alpha, const float *B, float beta, float *C,
                      int rp_time, double *elapsed_ns);

/* Device-resident form: all pointers are device pointers on the engine's device, column major
 * with explicit leading dimensions (ldb >= K, ldc >= M).  d_C_in and d_C_out may alias.
 * Enqueues on `stream` (a hipStream_t passed as void*) and returns without synchronising.  NULL = the CALLING THREAD's default
 * stream: the library is built with per-thread default streams (it never touches HIP's process-wide legacy stream, see
 * INTEGRATION.md section 9); that stream is a blocking stream, so it still orders itself after work the caller put on the legacy
 * stream. */
int sextans_spmm_device(sextans_handle_t h, int N, float alpha, const float *d_B, int64_t ldb,
                        float beta, const float *d_C_in, float *d_C_out, int64_t ldc, void *stream);

/* Same with separate leading dimensions for C_in and C_out (multi-GPU: a rank reads its rows of the
 * full column-major C_in, ldc_in = M, and writes a packed M_local x N slab, ldc_out = M_local). */
int sextans_spmm_device2(sextans_handle_t h, int N, float alpha, const float *d_B, int64_t ldb,
                         float beta, const float *d_C_in, int64_t ldc_in, float *d_C_out,
                         int64_t ldc_out, void *stream);

/* ROW-MAJOR operands (round 5): B is K x N with B[k * ldb + n], C_in / C_out are M x N with C[m * ldc + n] (ld >= N; C_in and C_out may
 * alias).  The reference lays B and C out for its kernel on the host, outside the timed call (sextans-host.cpp:150-195, 264-270); the
 * column-major entry points above pay for that inside the call (B repack; two more passes over C in the reordered form).  Here the
 * caller's B IS the kernel's panel (N = 16: exactly; N > 16: tile t = columns 16 t .. at row stride ldb) and C is read and written in
 * the caller's rows, 16 bytes per lane: no layout pass on the LDS-panel paths (natural-order, grid-brick and graph-clustered plans;
 * sextans_last_kernel = "spmm_csr_panel_v2_rowmajor[_clustered]") nor on the lane-per-row kernel ("spmm_csr_colwise_rowmajor"), and a
 * graph-clustered plan is used from 25 % fewer panel rows on instead of 40 %.  Needs 16-byte aligned pointers and ld % 4 == 0 (panel
 * paths: also K * ldb < 2^32 and M * ldc < 2^30); everything else (gather kernel, rows on the long-row paths, dense tiles on MFMA,
 * unaligned operands, N = 512 on 4 M rows) goes through column-major copies in the engine's workspaces.  Same arithmetic, same order:
 * bit-identical to cpu_spmm_CSR. */
int sextans_spmm_device_rm(sextans_handle_t h, int N, float alpha, const float *d_B, int64_t ldb, float beta, const float *d_C_in,
                           int64_t ldc_in, float *d_C_out, int64_t ldc, void *stream);

/* Everything the first SpMM call for (matrix, options, N, layout) would build inside itself -- packed row-bucketed plan, clustered row
 * order, long-row tables, workspaces, side streams -- built NOW, outside any timed region or hipGraph capture (round 6).  The
 * analogue of the reference preparing its streams before tapa::invoke (sextans-host.cpp:114-204).  Optional: the compute entry
 * points prepare lazily.  `stream` is only used for the few device passes of the builders (it is synchronised). */
#define SEXTANS_LAYOUT_COLMAJOR 0
#define SEXTANS_LAYOUT_ROWMAJOR 1
/* SEXTANS_LAYOUT_ROWMAJOR_T: the backward-pass forms -- A^T (sextans_csr_transpose_device) and everything the row-major calls of
 * sextans_spmm_t_device_rm build (plans, workspaces) on the companion engine, the row table of sextans_sddmm_device_rm and the tables of sextans_row_softmax_device -- those of A and, for the column pass of
 * sextans_attention_backward_device, those of A^T.  After it, a transposed call for N, an SDDMM call, a row-softmax call and the fused attention calls allocate nothing
 * and do not synchronise with the host: they may be captured into a hipGraph.  (Layout 2 is unused.) */
#define SEXTANS_LAYOUT_ROWMAJOR_T 3
int sextans_prepare(sextans_handle_t h, int N, int layout, void *stream);

/* New VALUES for the pattern currently set on h, without planning again: nnz floats in the CSR entry order the matrix was set with
 * (the "numeric phase" of a Newton / time-stepping / training loop; sextans_set_matrix_* + sextans_prepare are the "analysis phase").
 * Planning depends on the pattern and the options alone, so everything built from the pattern stays -- block dictionaries and index
 * lists, grid-brick and graph clustering, column relabelling, long-row tables, the sort behind A^T, the SDDMM row table -- and only the
 * copies of the values are rewritten.  Afterwards every compute entry point and sextans_export_plan behave exactly as on a fresh engine
 * with the same options and the new values: same kernel (sextans_last_kernel), same bits.
 *   sextans_update_values_device  matrix set with sextans_set_matrix_csr_device: d_val BECOMES the engine's value array (not copied, not
 *       owned; it may be the pointer as before = "changed in place").  Matrix the engine owns (sextans_set_matrix_csr / _edges): copied
 *       into the owned array on `stream`.  Then every value-bearing form that exists at that moment is rewritten on `stream` (NULL: the
 *       calling thread's default stream); forms not built yet are built later from the live array, as always.
 *   sextans_update_values         host values: uploaded (synchronous, like sextans_set_matrix_csr; for a caller-provided device matrix
 *       into an array the engine owns from then on), then the same.
 * With default options in both accuracy modes -- natural / grid-brick / graph-clustered plans at every lanes_per_row including the parked
 * ones, the mixed-plan split form, the main matrix behind the long-row split, the chain copy of the reordered form, A^T (through the
 * entry permutation kept from its sort, 4 bytes per non-zero, in "device_bytes") and recursively its companion engine -- the device call
 * ALLOCATES NOTHING, READS NOTHING BACK AND DOES NOT SYNCHRONISE: it enqueues copy kernels (value_refresh_kernels.h) and returns, so it
 * can be captured into a hipGraph together with the SpMM that follows.  The opt-in forms that hold transformed values -- the window
 * stream ("kernel" = 3), dense tiles / routed row blocks ("mfma_dense_tiles" = 1 / 2: then everything downstream of the matrix as set)
 * -- are DROPPED instead and rebuilt by the next call that needs them: correct, but that call plans, allocates and synchronises again.
 * Stats: "value_refreshes" (updates served on this matrix), "value_refresh_rebuilt" (how many of them dropped a form); both reset by
 * sextans_set_matrix_*.  "plan_build_s", "transpose_build_s", sextans_reassociated_rows and the clustering stats do not change.
 * SEXTANS_ERR_INVALID: h == NULL, or values NULL with nnz > 0; SEXTANS_ERR_STATE: no CSR matrix set (the blocked-ELL bf16 matrix of
 * sextans_set_matrix_bell* is not covered); nnz == 0: OK, nothing to do.  A changed PATTERN still needs sextans_set_matrix_*. */
int sextans_update_values_device(sextans_handle_t h, const float *d_val, void *stream);
int sextans_update_values(sextans_handle_t h, const float *val);

/* ---- Backward products (torch autograd of C = alpha * A * B + beta * C_in: dB = alpha * A^T * G, dA = alpha * (G * B^T) on A's pattern).
 *
 * Stable device transpose: the CSR of A^T (K x M) as new device arrays on `device` (sextans_device_free each), byte-identical to what the
 * reference's CSC_2_CSR (sparse_helper.h:475-509) makes of A's CSR read as the CSC of A^T -- inside a row of A^T the entries come in
 * ascending row of A and, for duplicate (row, column) entries, in storage order.  One stable radix sort of (column, entry) pairs: no atomics,
 * the same bits on every run.  Empty rows / columns, M, K or nnz = 0 and duplicates are fine; nnz < 2^31; columns are validated
 * (SEXTANS_ERR_INDEX outside [0, K)).  Enqueued on `stream` (NULL: the calling thread's default stream), which is synchronised. */
int sextans_csr_transpose_device(int device, int M, int K, int64_t nnz, const int *d_row_ptr, const int *d_col_idx, const float *d_val,
                                 int **o_row_ptr, int **o_col_idx, float **o_val, void *stream);

/* C (K x N) = alpha * A^T * B + beta * C_in for the matrix set on h; B is M x N, every operand ROW-major, argument rules of
 * sextans_spmm_device_rm (ld >= N, N % 8 == 0, C_in may alias C_out; unaligned operands take that entry point's fallback).
 * The handle builds A^T once (sextans_csr_transpose_device) and holds it in an internal companion engine whose sextans_spmm_device_rm
 * serves the call: A^T gets every path of the dispatcher (panel, clustered, gather, lane-per-row, long-row chains).  No atomic scatter:
 *   SEXTANS_MODE_STRICT  bit-identical to cpu_spmm_CSR on CSC_2_CSR(A) (the arrays of sextans_csr_transpose_device);
 *   SEXTANS_MODE_FAST    the tolerance stated with the modes (bit-equal to the fmaf chain on matrices without hub rows).
 * Lifecycle: built by the first transposed call or by sextans_prepare(h, N, SEXTANS_LAYOUT_ROWMAJOR_T, stream); dropped by
 * sextans_set_matrix_*, freed by sextans_destroy.  A^T's VALUES ARE A SNAPSHOT taken when it is built (as the packed plans of A are): a
 * caller that changes A's values in place calls sextans_update_values_device, which refreshes A^T and the companion's forms too.  Every sextans_set_option on h applies to the transposed form too, also
 * later ones, with the same validation -- except "row_offset" and "global_nnz" (row slabs of the multi-GPU forms).  sextans_last_kernel(h)
 * names the kernel the call ran; stat "device_bytes" includes A^T ((K + 1) * 4 + nnz * 8 bytes) and the companion's plans and workspaces;
 * stat "transpose_build_s" = seconds spent building A^T and its plans. */
int sextans_spmm_t_device_rm(sextans_handle_t h, int N, float alpha, const float *d_B, int64_t ldb, float beta, const float *d_C_in,
                             int64_t ldc_in, float *d_C_out, int64_t ldc, void *stream);

/* SDDMM on A's pattern, row-major X (M x N, X[r * ldx + n]) and Y (K x N): for every stored entry e = (r, c) of the matrix set on h, in
 * the CSR entry order it was set with (not a plan's order):
 *     acc = +0.0f;  for n = 0 .. N-1: acc = acc + X[r, n] * Y[c, n]      (every product and every sum rounded to fp32, no FMA)
 *     out[e] = d_vals_in ? alpha * acc + beta * vals_in[e] : alpha * acc   (each product and the sum rounded: cpu_spmm_CSR's epilogue)
 * -- cpu_spmm_CSR's rounding (sparse_helper.h:262-290) applied to a dot product, in EVERY mode.  d_vals_in may be NULL (not read) or alias
 * d_vals_out.  Needs N % 8 == 0, ldx, ldy >= N with ld % 4 == 0 and 16-byte aligned d_X, d_Y, d_vals_in, d_vals_out; anything else is
 * SEXTANS_ERR_INVALID (no fallback).  Work is split by non-zeros (hub rows spread over many wavefronts), no atomics; enqueued on `stream`.
 * The first call on a matrix validates it (matrices set with sextans_set_matrix_csr_device) and builds a table of the row of every
 * 256-entry range (nnz / 64 bytes, in stat "device_bytes"); later calls allocate nothing and do not synchronise with the host.
 * sextans_prepare(h, N, SEXTANS_LAYOUT_ROWMAJOR_T, stream) builds it ahead, with the transposed form. */
int sextans_sddmm_device_rm(sextans_handle_t h, int N, float alpha, const float *d_X, int64_t ldx, const float *d_Y, int64_t ldy, float beta,
                            const float *d_vals_in, float *d_vals_out, void *stream);

/* ---- Row softmax on A's pattern (the step between the SDDMM and the SpMM of attention over a fixed sparsity pattern: graph attention,
 * sparse / sliding-window attention).  Closest thing in the reference: none -- its PEs only multiply and accumulate.
 *
 * For the CSR matrix set on h, for every row r with stored entries e in [row_ptr[r], row_ptr[r + 1]), in the entry order it was set with:
 *     forward    s_e = scale * x_e;   m = max_e s_e;   t_e = exp(s_e - m);   Z = sum_e t_e;   p_e = t_e / Z
 *     backward   d = sum_e p_e * g_e;   dx_e = scale * p_e * (g_e - d)
 * in fp32: every product and difference rounded once, exp as exp2 of a rounded product, the sums as fixed trees (at most 32 consecutive
 * adds per lane, then cross-lane butterflies; long rows: per-chunk partial results combined in a fixed order), p_e = t_e * (1 / Z).  The
 * same arithmetic in SEXTANS_MODE_STRICT and SEXTANS_MODE_FAST; no float atomics: the same call gives the same bits on every run and
 * every stream.  Special values as torch.softmax over the row's stored entries: a -inf entry beside finite ones gives exactly +0.0f; a
 * row of only -inf, a +inf or a NaN gives NaN for the whole row; an empty row does nothing; a row of one finite entry gives exactly
 * 1.0f (backward: dx = +-0).  A's VALUES are not read: only its pattern.
 * d_x, d_p, d_g, d_dx: nnz floats each in the CSR entry order of the matrix as set -- the order sextans_sddmm_device_rm writes and
 * sextans_update_values_device reads, so SDDMM -> softmax -> value refresh -> SpMM chain without a permutation.  16-byte aligned.
 * Aliasing: d_p may be d_x (in place); d_dx may be d_g or d_p; any other overlap is undefined.
 * Work is split by non-zeros (a wavefront owns whole rows of about 256 entries in all; a row stays in registers between the max, the
 * sum and the normalisation: 8 bytes of traffic per non-zero forward, 12 backward); rows longer than 2048 entries take a long-row path
 * (2048-entry chunks on a wavefront each, partial results in a workspace, one more read of those rows).  The first call on a matrix
 * validates it (matrices set with sextans_set_matrix_csr_device), builds the tables (nnz / 64 bytes + 24 bytes per long-row chunk, in
 * stat "device_bytes") and synchronises; sextans_prepare(h, N, SEXTANS_LAYOUT_ROWMAJOR_T, stream) builds them ahead.  After either, a
 * call allocates nothing, reads nothing back and does not synchronise: it can be captured into a hipGraph.  The tables depend on the
 * pattern alone: sextans_update_values* leaves them, sextans_set_matrix_* drops them.  Calls on one handle share the long-row
 * workspace: run them on one stream, or order them.
 * sextans_last_kernel: "row_softmax" / "row_softmax_backward", "+long_rows" appended when the long-row path ran; stat
 * "softmax_long_rows": rows on it (0 before the tables exist).
 * SEXTANS_ERR_INVALID: h == NULL, a misaligned pointer, a NULL pointer with nnz > 0; SEXTANS_ERR_STATE: no CSR matrix set (the
 * blocked-ELL bf16 matrix is not covered); nnz == 0 or M == 0: OK, nothing to do. */
int sextans_row_softmax_device(sextans_handle_t h, float scale, const float *d_x, float *d_p, void *stream);
int sextans_row_softmax_backward_device(sextans_handle_t h, float scale, const float *d_p, const float *d_g, float *d_dx, void *stream);

/* ---- Fused multi-head attention on A's pattern: what sddmm -> row_softmax -> value refresh -> spmm computes per head, in one kernel
 * pass per direction for all heads, with nothing of size nnz written and no value refresh.  Closest thing in the reference: none.
 *
 * Operands are ROW-major fp32 with the heads side by side in a row: Q is M x (heads * d), head h in columns [h * d, (h + 1) * d) -- a
 * contiguous (M, heads, d) array --, K is K x (heads * d), V is K x (heads * dv), O and G are M x (heads * dv); lse and delta are
 * M x heads, dense.  Every operand has its own leading dimension (floats between rows).  d_bias: NULL, or nnz floats in the CSR entry
 * order the matrix was set with, shared by all heads -- an explicit pointer: A's own VALUES ARE NEITHER READ NOR WRITTEN.
 * For every row r, head h and stored entry e = (r, c):
 *     forward    s_e = scale * (<Q[r,h,:], K[c,h,:]> + bias_e);   m = max_e s_e;   Z = sum_e exp(s_e - m)
 *                O[r,h,:] = (sum_e exp(s_e - m) * V[c,h,:]) / Z;   lse[r,h] = m + log Z
 *     backward   delta[r,h] = <O[r,h,:], G[r,h,:]>;   p_e = exp(s_e - lse[r,h]);   ds_e = p_e * (<G[r,h,:], V[c,h,:]> - delta[r,h])
 *                dQ[r,h,:] = sum_e scale ds_e K[c,h,:];   dK[c,h,:] = sum_e scale ds_e Q[r,h,:];   dV[c,h,:] = sum_e p_e G[r,h,:]
 *                dbias_e = sum_h scale ds_e   (d_dbias != NULL; heads added in ascending order)
 * The forward is an online softmax (a running m, Z and accumulator, rescaled when m grows); the backward recomputes p from lse in two
 * passes, rows of A for delta, dQ and dbias, rows of A^T (sextans_csr_transpose_device's arrays and entry permutation) for dK and dV.
 * fp32 throughout, FMA in the dot products and accumulations, exp as in the row softmax; every sum runs in an order fixed by the
 * pattern and the launch shape and there are no float atomics: the same call gives the same bits on every run and every stream.  The
 * same arithmetic in SEXTANS_MODE_STRICT and SEXTANS_MODE_FAST.  NOT BIT-EQUAL to the composition of sextans_sddmm_device_rm,
 * sextans_row_softmax_device and sextans_spmm_device_rm (which rounds every product and associates its sums differently): equal within
 * the tolerance of a chain of fp32 operations.
 * Special values as sextans_row_softmax_device: a -inf score beside finite ones contributes exactly 0; a row of only -inf scores, or
 * with a +inf or NaN score, gives NaN in that (row, head); an empty row writes O = +0 and lse = -inf.  Empty rows and columns get zero
 * gradients; every element of O, lse, delta, dQ, dK, dV (and dbias) is written.
 * d and dv: multiples of 8 in [8, 128]; both are served by one register width, the smallest of 8 / 16 / 32 / 64 / 128 floats that
 * holds the larger, with predicated loads.  Leading dimensions: >= heads * d (heads * dv), multiples of 4; every pointer 16-byte
 * aligned.  The outputs must not overlap the inputs or each other.
 * Work is dealt by non-zero count with the row softmax's tables (a group of lanes sized to the row takes a (row, head); K and V rows
 * come in as 16-byte gathers; the Q row and the accumulator stay in registers); rows -- in the column pass: columns -- of more than
 * 2048 entries get one workgroup per head whose four wavefronts are merged through LDS in a fixed order (one row is not split over
 * workgroups).  The first forward call on a matrix validates it and builds the row softmax's tables; the first backward call also
 * builds A^T (the arrays and the companion engine's tables only, none of its SpMM plans); both synchronise then.
 * sextans_prepare(h, N, SEXTANS_LAYOUT_ROWMAJOR_T, stream) builds all of it ahead.  After that a call allocates nothing, reads nothing
 * back and does not synchronise: it can be captured into a hipGraph.  Nothing is allocated beyond those tables (stat "device_bytes":
 * the terms of the row softmax and of A^T).
 * sextans_last_kernel: "attention_fused" / "attention_fused_backward", "+long_rows" appended when the workgroup path ran.
 * ("+dropout" comes before it from the dropout entries below.)
 * SEXTANS_ERR_INVALID: h == NULL, heads < 1, d or dv not a multiple of 8 in [8, 128], a leading dimension too small or not a multiple
 * of 4, a misaligned pointer, a NULL pointer other than d_bias / d_dbias with nnz > 0; SEXTANS_ERR_STATE: no CSR matrix set.  M == 0
 * or nnz == 0: OK -- O and the gradients are zeroed, lse = -inf. */
int sextans_attention_device(sextans_handle_t h, int heads, int d, int dv, float scale,
    const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk, const float *d_V, int64_t ldv,
    const float *d_bias, float *d_O, int64_t ldo, float *d_lse, void *stream);
int sextans_attention_backward_device(sextans_handle_t h, int heads, int d, int dv, float scale,
    const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk, const float *d_V, int64_t ldv,
    const float *d_bias, const float *d_O, int64_t ldo, const float *d_lse, const float *d_G, int64_t ldg,
    float *d_delta, float *d_dQ, int64_t lddq, float *d_dK, int64_t lddk, float *d_dV, int64_t lddv,
    float *d_dbias, void *stream);

/* ---- Fused graph attention (GAT, as GATConv in PyG / DGL) on A's pattern: the fused attention above with an ADDITIVE score and a
 * LeakyReLU in front of the softmax, in one kernel pass per direction for all heads.  Closest thing in the reference: none.
 *
 * An edge e = (r, c) -- source c, destination r -- is scored from two scalars per node and head instead of a dot product.  Operands are
 * ROW-major fp32: adst and dadst are M x heads, asrc and dasrc K x heads (entry [i * ld + h]; ld >= heads is the only condition on
 * these four leading dimensions: they are read and written one float at a time); V and dV are K x (heads * dv) with head h in columns
 * [h * dv, (h + 1) * dv), O and G are M x (heads * dv); lse and delta are M x heads, dense.  d_bias: NULL (bias_e = 0), or nnz floats
 * in the CSR entry order the matrix was set with, shared by all heads -- an explicit pointer: A's own VALUES ARE NEITHER READ NOR
 * WRITTEN.  For every row r, head h and stored entry e = (r, c), in entry order:
 *     forward    z_e = (adst[r,h] + asrc[c,h]) + bias_e          (this order of the two adds)
 *                s_e = z_e > 0 ? z_e : negative_slope * z_e       (a -inf z stays -inf for every slope, 0 included; NaN stays NaN)
 *                m = max_e s_e;   Z = sum_e exp(s_e - m);   O[r,h,:] = (sum_e exp(s_e - m) * V[c,h,:]) / Z;   lse[r,h] = m + log Z
 *     backward   delta[r,h] = <O[r,h,:], G[r,h,:]>;   p_e = exp(s_e - lse[r,h]);   ds_e = p_e * (<G[r,h,:], V[c,h,:]> - delta[r,h])
 *                dz_e = z_e > 0 ? ds_e : negative_slope * ds_e    (z == 0 takes the slope, as torch's leaky_relu backward)
 *                dadst[r,h] = sum_e dz_e;   dasrc[c,h] = sum_e dz_e;   dV[c,h,:] = sum_e p_e G[r,h,:]
 *                dbias_e = sum_h dz_e   (d_dbias != NULL; heads added in ascending order)
 * The forward is an online softmax (a running m, Z and accumulator, rescaled when m grows); the backward recomputes z and p from lse
 * in two passes, rows of A for delta, dadst and dbias, rows of A^T (sextans_csr_transpose_device's arrays and entry permutation) for
 * dasrc and dV.  Nothing of size nnz is read or written besides bias and dbias.
 * Arithmetic and determinism: fp32 throughout, FMA in the dot products <O, G>, <G, V> and in the V / G accumulations, exp as in the row
 * softmax (exp2 of a rounded product); every sum runs in an order fixed by the pattern and the launch shape and there are no float
 * atomics: the same call gives the same bits on every run and every stream.  The same arithmetic in SEXTANS_MODE_STRICT and
 * SEXTANS_MODE_FAST.
 * Special values: a -inf score (a -inf bias: a mask) beside finite ones contributes exactly 0, to O and to every gradient; a row of only
 * -inf scores, or with a +inf or NaN score, gives NaN in that (row, head); an empty row writes O = +0 and lse = -inf.  Empty rows and
 * columns get zero gradients; every element of O, lse, delta, dadst, dasrc, dV (and dbias) is written.
 * dv: a multiple of 8 in [8, 128]; it alone sets the register width, the smallest of 8 / 16 / 32 / 64 / 128 floats that holds it.
 * negative_slope: finite and >= 0 (1 makes the activation the identity).  Leading dimensions of V, O, G, dV: >= heads * dv, multiples of
 * 4; every pointer 16-byte aligned.  The outputs must not overlap the inputs or each other.
 * Work is dealt by non-zero count with the row softmax's tables exactly as in sextans_attention_device (a group of lanes sized to the
 * row takes a (row, head); per entry one 4-byte load and one gathered V -- column pass: G -- row; rows or columns of more than 2048
 * entries get one workgroup per head, merged through LDS in a fixed order).  The first forward call on a matrix validates it and
 * builds the row softmax's tables; the first backward call also builds A^T (its arrays and the companion engine's tables only); both
 * synchronise then.  sextans_prepare(h, N, SEXTANS_LAYOUT_ROWMAJOR_T, stream) builds all of it ahead.  After either, a call allocates
 * nothing, reads nothing back and does not synchronise: it can be captured into a hipGraph.  Nothing is allocated beyond those tables
 * (stat "device_bytes": the terms of the row softmax and of A^T).
 * sextans_last_kernel: "gat_fused" / "gat_fused_backward", "+long_rows" appended when the workgroup path ran.
 * ("+dropout" comes before it from the dropout entries below.)
 * SEXTANS_ERR_INVALID: h == NULL, heads < 1, dv not a multiple of 8 in [8, 128], negative_slope negative, NaN or infinite, ldadst /
 * ldasrc / lddadst / lddasrc < heads, another leading dimension too small or not a multiple of 4, a misaligned pointer -- checked in
 * this order, then the handle's state (SEXTANS_ERR_STATE: no CSR matrix set), then SEXTANS_ERR_INVALID for a NULL pointer other than
 * d_bias / d_dbias with nnz > 0: the order of sextans_attention_device, all before any device is touched.  M == 0 or nnz == 0: OK -- O
 * and the gradients are zeroed, lse = -inf. */
int sextans_gat_attention_device(sextans_handle_t h, int heads, int dv, float negative_slope,
    const float *d_adst, int64_t ldadst, const float *d_asrc, int64_t ldasrc, const float *d_V, int64_t ldv,
    const float *d_bias, float *d_O, int64_t ldo, float *d_lse, void *stream);
int sextans_gat_attention_backward_device(sextans_handle_t h, int heads, int dv, float negative_slope,
    const float *d_adst, int64_t ldadst, const float *d_asrc, int64_t ldasrc, const float *d_V, int64_t ldv,
    const float *d_bias, const float *d_O, int64_t ldo, const float *d_lse, const float *d_G, int64_t ldg,
    float *d_delta, float *d_dadst, int64_t lddadst, float *d_dasrc, int64_t lddasrc, float *d_dV, int64_t lddv,
    float *d_dbias, void *stream);

/* ---- Fused GATv2 graph attention (as GATv2Conv in PyG / DGL) on A's pattern: the score's activation sits INSIDE the projection, so no
 * pair of per-node scalars expresses it; the message is the gathered source row itself.  One kernel pass per direction for all heads.
 * Closest thing in the reference: none.
 *
 * Operands are ROW-major fp32 with the heads side by side in a row: x_dst, dx_dst, O and G are M x (heads * d), x_src and dx_src are
 * K x (heads * d), head h in columns [h * d, (h + 1) * d); att and datt are heads * d floats, contiguous; lse and delta are M x heads,
 * dense.  d_bias: NULL (bias_e = 0), or nnz floats in the CSR entry order the matrix was set with, shared by all heads -- an explicit
 * pointer: A's own VALUES ARE NEITHER READ NOR WRITTEN.  For every row r, head h and stored entry e = (r, c):
 *     forward    z_e[k] = x_dst[r,h,k] + x_src[c,h,k]                      (one rounded add, the same bits in every pass)
 *                l_e[k] = z_e[k] > 0 ? z_e[k] : negative_slope * z_e[k]     (plain LeakyReLU: the mask is the bias, not z)
 *                s_e = <att[h,:], l_e> + bias_e                             (the bias is added after the dot product)
 *                m = max_e s_e;   Z = sum_e exp(s_e - m);   O[r,h,:] = (sum_e exp(s_e - m) * x_src[c,h,:]) / Z;   lse[r,h] = m + log Z
 *     backward   delta[r,h] = <O[r,h,:], G[r,h,:]>;   p_e = exp(s_e - lse[r,h]);   ds_e = p_e * (<G[r,h,:], x_src[c,h,:]> - delta[r,h])
 *                g_e[k] = ds_e * att[h,k] * (z_e[k] > 0 ? 1 : negative_slope)   (z == 0 takes the slope, as torch's leaky_relu backward)
 *                dx_dst[r,h,:] = sum_e g_e;   dx_src[c,h,:] = sum_e (p_e G[r,h,:] + g_e);   dbias_e = sum_h ds_e   (d_dbias != NULL)
 *                datt_rows[r,h,:] = sum_e ds_e l_e;   datt[h,k] = sum_r datt_rows[r,h,k]
 * There is no separate V operand: the message is x_src, as in GATv2Conv.  x_dst and x_src may be the same array (a square pattern with
 * shared weights); the two gradients are still written separately and the caller adds them.
 * The sum over r in datt runs in a FIXED two-level order that defines its bits: part[c, j] adds the rows 256 c, 256 c + 1, .. of chunk c
 * in ascending order starting from +0, datt[j] adds part[0, j], part[1, j], .. in ascending order starting from +0, every add rounded to
 * nearest.  d_work: sextans_gatv2_workspace_floats(h, heads, d) = M * heads * d + ceil(M / 256) * heads * d floats handed in by the
 * caller; after the call it holds datt_rows (M x (heads * d), dense) followed by part (ceil(M / 256) x (heads * d)).  d_delta: M * heads
 * floats, written.
 * Arithmetic and determinism as sextans_gat_attention_device: fp32 throughout, FMA in the dot products and accumulations, exp as in the
 * row softmax, no float atomics, the same bits on every run and every stream, the same arithmetic in both modes.  Special values: a
 * -inf bias beside finite ones contributes exactly 0 to O and to every gradient; a row of only -inf scores, or with a +inf or NaN
 * score, gives NaN in that (row, head); an empty row writes O = +0, lse = -inf and zero gradient and datt_rows rows; columns without
 * entries get zero dx_src rows.
 * d: a multiple of 8 in [8, 128]; it alone sets the register width (8 / 16 / 32 / 64 / 128 floats).  negative_slope: finite and >= 0.
 * Leading dimensions: >= heads * d, multiples of 4; every pointer 16-byte aligned.  The outputs must not overlap the inputs or each
 * other.  Work is dealt exactly as in sextans_attention_device; per entry the forward and the row pass gather ONE row (x_src[c]: score
 * operand and message at once), the column pass two (x_dst[r], G[r]).  Tables, the first calls' synchronisation, sextans_prepare and
 * hipGraph capture as for sextans_gat_attention_device: after the first backward call nothing is allocated, read back or synchronised.
 * sextans_last_kernel: "gatv2_fused" / "gatv2_fused_backward", "+long_rows" appended when the workgroup path ran.
 * ("+dropout" comes before it from the dropout entries below.)
 * SEXTANS_ERR_INVALID: h == NULL, heads < 1, d not a multiple of 8 in [8, 128], negative_slope negative, NaN or infinite, a leading
 * dimension too small or not a multiple of 4, a misaligned pointer -- checked in this order, then the handle's state (SEXTANS_ERR_STATE:
 * no CSR matrix set), then SEXTANS_ERR_INVALID for a NULL pointer other than d_bias / d_dbias with nnz > 0; all before any device is
 * touched.  sextans_gatv2_workspace_floats returns the error code negated.  M == 0 or nnz == 0: OK -- O, the gradients, datt and the
 * workspace are zeroed, lse = -inf. */
int64_t sextans_gatv2_workspace_floats(sextans_handle_t h, int heads, int d);
int sextans_gatv2_attention_device(sextans_handle_t h, int heads, int d, float negative_slope,
    const float *d_xdst, int64_t ldxd, const float *d_xsrc, int64_t ldxs, const float *d_att,
    const float *d_bias, float *d_O, int64_t ldo, float *d_lse, void *stream);
int sextans_gatv2_attention_backward_device(sextans_handle_t h, int heads, int d, float negative_slope,
    const float *d_xdst, int64_t ldxd, const float *d_xsrc, int64_t ldxs, const float *d_att,
    const float *d_bias, const float *d_O, int64_t ldo, const float *d_lse, const float *d_G, int64_t ldg,
    float *d_delta, float *d_dxdst, int64_t lddxd, float *d_dxsrc, int64_t lddxs, float *d_datt, float *d_work,
    float *d_dbias, void *stream);

/* ---- Attention dropout inside the three fused attentions above: dropout on the NORMALISED attention coefficients (GATConv / GATv2Conv's
 * dropout in PyG and DGL, attn_drop of graph transformers), which the fused kernels never materialise.  The mask is made inside the
 * kernels by a counter-based generator and recomputed by all three passes: no state of size nnz, no atomics, the same bits on every
 * run, capturable.  Closest thing in the reference: none.
 *
 * With m_e,h = 1 / (1 - p) where (entry e, head h) is kept and 0 where it is dropped -- scores, m, Z, lse and p_e = exp(s_e - lse) stay
 * exactly as in the entries without dropout (dropped entries still count in Z, so the special-value rules are unchanged):
 *     forward    O[r,h,:] = sum_e (m_e p_e) V[c,h,:]                         (GATv2: x_src[c,h,:])
 *     backward   delta[r,h] = <O[r,h,:], G[r,h,:]>   (the dropped O: sum_e p_e m_e <G, V_e> = <O, G>)
 *                ds_e = p_e * (m_e * <G[r,h,:], V[c,h,:]> - delta[r,h])
 *                dV[c,h,:] = sum_e (m_e p_e) G[r,h,:]                        (GATv2: the p_e G term of dx_src)
 * and everything downstream of ds_e as before (dQ, dK, dz, dadst, dasrc, g_e, dx_dst, datt_rows, datt, dbias).  m_e p_e and
 * m_e <G, V> are one rounded multiply each.  A row whose entries are all dropped gives O = +0, lse as without dropout, and zero ds_e.
 * The mask (csrc/dropout_hash.h; uint64 arithmetic wraps):
 *     mix(x):  x += 0x9E3779B97F4A7C15;  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;  x = (x ^ (x >> 27)) * 0x94D049BB133111EB;  x ^ (x >> 31)
 *     key  = mix(seed + step)                        step = *d_step, or 0 when d_step == NULL
 *     u    = (uint32)(mix(key + e * heads + h) >> 32)   e: the entry's position in the CSR arrays as set (also in the column pass), h: head
 *     keep = u >= thresh,  thresh = (uint32)((double)p * 4294967296.0);   m = keep ? 1.0f / (1.0f - p) : 0.0f   (two rounded fp32 operations)
 * d_step: NULL, or ONE 8-byte aligned uint64 in device memory that every thread reads once.  It exists so that a captured hipGraph
 * draws a new mask on each replay: the caller bumps the word between replays (on the stream); nothing is read back or synchronised.
 * The backward call must get the p, seed and step of its forward.
 * drop == NULL or p == 0: exactly the entry without "_dropout" -- the same kernels, the same bits.  p > 0 launches a compile-time
 * variant of the same kernels (the same row walking, lane groups, long-row workgroups, merges and order of every sum) that costs two
 * 64-bit multiplies per (entry, head) and slot lane; sextans_last_kernel then carries "+dropout" (before "+long_rows").
 * SEXTANS_ERR_INVALID additionally for p negative, NaN or >= 1 and a misaligned d_step, checked right after heads, the head
 * dimensions and negative_slope (scale has no check) and before the leading dimensions; everything else as the entries without dropout.
 * sextans_dropout_mask_device writes the nnz * heads multipliers m, [e * heads + h], of the handle's matrix (what the fused kernels
 * recompute; for compositions that materialise the coefficients, and for tests); drop must not be NULL, d_mult 16-byte aligned.
 * sextans_dropout_keep_host needs no device and no handle: keep[i * heads + h] = 1 where (entry first + i, head h) is kept, for
 * i in [0, count); SEXTANS_ERR_INVALID for first or count negative, heads < 1, a bad p, keep == NULL with count > 0. */
typedef struct { float p; uint64_t seed; const uint64_t *d_step; } sextans_dropout;
int sextans_attention_dropout_device(sextans_handle_t h, int heads, int d, int dv, float scale,
    const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk, const float *d_V, int64_t ldv,
    const float *d_bias, float *d_O, int64_t ldo, float *d_lse, const sextans_dropout *drop, void *stream);
int sextans_attention_dropout_backward_device(sextans_handle_t h, int heads, int d, int dv, float scale,
    const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk, const float *d_V, int64_t ldv,
    const float *d_bias, const float *d_O, int64_t ldo, const float *d_lse, const float *d_G, int64_t ldg,
    float *d_delta, float *d_dQ, int64_t lddq, float *d_dK, int64_t lddk, float *d_dV, int64_t lddv,
    float *d_dbias, const sextans_dropout *drop, void *stream);
int sextans_gat_attention_dropout_device(sextans_handle_t h, int heads, int dv, float negative_slope,
    const float *d_adst, int64_t ldadst, const float *d_asrc, int64_t ldasrc, const float *d_V, int64_t ldv,
    const float *d_bias, float *d_O, int64_t ldo, float *d_lse, const sextans_dropout *drop, void *stream);
int sextans_gat_attention_dropout_backward_device(sextans_handle_t h, int heads, int dv, float negative_slope,
    const float *d_adst, int64_t ldadst, const float *d_asrc, int64_t ldasrc, const float *d_V, int64_t ldv,
    const float *d_bias, const float *d_O, int64_t ldo, const float *d_lse, const float *d_G, int64_t ldg,
    float *d_delta, float *d_dadst, int64_t lddadst, float *d_dasrc, int64_t lddasrc, float *d_dV, int64_t lddv,
    float *d_dbias, const sextans_dropout *drop, void *stream);
int sextans_gatv2_attention_dropout_device(sextans_handle_t h, int heads, int d, float negative_slope,
    const float *d_xdst, int64_t ldxd, const float *d_xsrc, int64_t ldxs, const float *d_att,
    const float *d_bias, float *d_O, int64_t ldo, float *d_lse, const sextans_dropout *drop, void *stream);
int sextans_gatv2_attention_dropout_backward_device(sextans_handle_t h, int heads, int d, float negative_slope,
    const float *d_xdst, int64_t ldxd, const float *d_xsrc, int64_t ldxs, const float *d_att,
    const float *d_bias, const float *d_O, int64_t ldo, const float *d_lse, const float *d_G, int64_t ldg,
    float *d_delta, float *d_dxdst, int64_t lddxd, float *d_dxsrc, int64_t lddxs, float *d_datt, float *d_work,
    float *d_dbias, const sextans_dropout *drop, void *stream);
int sextans_dropout_mask_device(sextans_handle_t h, int heads, const sextans_dropout *drop, float *d_mult, void *stream);
int sextans_dropout_keep_host(int64_t first, int64_t count, int heads, float p, uint64_t seed, uint64_t step, uint8_t *keep);

/* ---- Max / min aggregation SpMM: C = A (x) B with the row's SUM replaced by its maximum or minimum, and the entries that won (what
 * torch.sparse.mm(A, B, "amax" / "amin") computes on the CPU, reduce="max" in PyG, copy_u_max in DGL).  Closest thing in the reference:
 * none.
 *
 * A is the engine's M x K CSR pattern, B row-major K x N fp32 (B[k * ldb + n]), C row-major M x N fp32, arg row-major M x N int32.
 * d_val: nnz floats in the CSR entry order the matrix was set with -- an explicit pointer like the attention entries' bias; NULL = the
 * engine's current values (as set, or as of the last sextans_update_values*).  No value refresh happens and none of the engine's packed
 * forms is read or written.  For every row r and column n, over the stored entries e = (r, c) of the row:
 *     forward    p_e = val[e] * B[c, n]                           (one fp32 product rounded to nearest, never fused)
 *                C[r, n] = max_e p_e (SEXTANS_REDUCE_MAX) / min_e p_e (SEXTANS_REDUCE_MIN);   arg[r, n] = the winning e, its position in
 *                the CSR arrays.  Among equal products the SMALLEST e wins (+0 and -0 compare equal: the first one wins); if any p_e is
 *                NaN, C[r, n] is that NaN and arg the smallest e with a NaN product.  A row without stored entries: C = +0, arg = -1.
 *                Stored explicit zeros take part like any entry.  (np.argmax / np.argmin over the row's (entries x N) product block.)
 *     backward   dB[c, n]  = sum over the entries e of column c whose row r has arg[r, n] == e of val[e] * G[r, n]
 *                dval[e]   = sum over the n with arg[r, n] == e of G[r, n] * B[c, n]
 *                (a tied or NaN position sends its gradient to the one winner, as torch's CPU kernel does)
 * C and arg are BIT-DETERMINED by these rules: every product is rounded on its own and the comparison (is NaN, product, entry) is a
 * total order, so they do not depend on how a row is split over lanes, wavefronts or the long-row workgroup, nor on the mode.  The
 * backward sums use FMA and run in an order fixed by the pattern and the launch shape; there are no atomics anywhere: dB is a GATHER
 * over the rows of A^T (sextans_csr_transpose_device's arrays and entry permutation), dval a row pass in which one lane owns an entry.
 * The same call gives the same bits on every run and every stream.
 * N: a multiple of 8, at least 8, no upper limit but 65535 tiles: the columns are cut into tiles of the smallest of 8 / 16 / 32 / 64 /
 * 128 floats that holds min(N, 128), which play the part the heads play in sextans_attention_device (a group of lanes sized to the row
 * takes a (row, tile); per entry one 4-byte column load, one 4-byte value load and the 16-byte pieces of one gathered B row; rows --
 * column pass: columns -- of more than 2048 entries get one workgroup per tile, merged through LDS).  The last tile may be partial.
 * Leading dimensions: >= N, multiples of 4 (all of them, whether or not their pointer is NULL); every pointer 16-byte aligned.  The
 * outputs must not overlap the inputs or each other.
 * d_arg may be NULL in the forward (inference).  In the backward d_dB or d_dval may be NULL, not both; d_B may be NULL when d_dval is.
 * The backward writes every element of dB (K x N) and of dval (nnz) it is given: columns without entries get zeros.
 * The first forward call on a matrix validates it and builds the row softmax's tables; the first backward call with d_dB also builds
 * A^T (its arrays and the companion engine's tables only); both synchronise then.  After that a call allocates nothing, reads nothing
 * back and does not synchronise: it can be captured into a hipGraph.  Nothing is allocated beyond those tables (stat "device_bytes":
 * the terms of the row softmax and of A^T).
 * sextans_last_kernel: "spmm_reduce" / "spmm_reduce_backward", "+long_rows" appended when the workgroup path ran.
 * SEXTANS_ERR_INVALID: h == NULL, op not SEXTANS_REDUCE_MAX / _MIN, N < 8 or not a multiple of 8, a leading dimension below N or not a
 * multiple of 4, a misaligned pointer, (backward) d_dB and d_dval both NULL -- checked in this order, then the handle's state
 * (SEXTANS_ERR_STATE: no CSR matrix set), then SEXTANS_ERR_INVALID for nnz > INT32_MAX and for a required pointer that is NULL with
 * nnz > 0; all before any device is touched.  M == 0 or nnz == 0: OK -- C and dB are zeroed, arg = -1. */
#define SEXTANS_REDUCE_MAX 1
#define SEXTANS_REDUCE_MIN 2
int sextans_spmm_reduce_device_rm(sextans_handle_t h, int op, int N, const float *d_val, const float *d_B, int64_t ldb,
                                  float *d_C, int64_t ldc, int32_t *d_arg, int64_t ldarg, void *stream);
int sextans_spmm_reduce_backward_device_rm(sextans_handle_t h, int N, const float *d_val, const float *d_B, int64_t ldb,
                                           const int32_t *d_arg, int64_t ldarg, const float *d_G, int64_t ldg,
                                           float *d_dB, int64_t lddb, float *d_dval, void *stream);

/* ---- Several aggregations of the SAME messages in one pass (PNA's mean / max / min / std, PyG's MultiAggregation, the mean || max
 * read-outs of GraphSAGE variants).  Closest thing in the reference: none.
 *
 * A, B, d_val and the message p_e[n] = val[e] * B[c, n] (ONE rounded fp32 product) are those of sextans_spmm_reduce_device_rm above; one
 * gathered B row per entry serves every aggregate.  Outputs (each row-major M x N with its OWN pointer and leading dimension, so that they
 * may be column slices of one (M, k N) buffer -- the concatenation PNA wants is written in place; columns beyond N are never written):
 *     d_sum      sum_e p_e                       (fp32 adds rounded to nearest)
 *     d_sumsq    sum_e p_e^2                     (s = fma(p_e, p_e, s))
 *     d_max / d_argmax, d_min / d_argmin          the values AND BITS of sextans_spmm_reduce_device_rm with SEXTANS_REDUCE_MAX / _MIN
 *     a row without stored entries: sums +0, max and min +0, args -1
 * The sums run in an order fixed by the pattern and the launch shape (no atomics: the same bits on every run and stream); that order does
 * not depend on which outputs are requested.  A NULL output is not computed (sum and sumsq form one group, max and min with their args
 * the other; a group without any pointer is compiled out) -- at least one of the four values must be given, and an arg needs its value.
 * Backward, for the upstream gradients that are given (NULL: absent) and the args of the forward:
 *     t_e[n]   = Gsum[r, n] + 2 p_e[n] Gsq[r, n] + (argmax[r, n] == e ? Gmax[r, n] : 0) + (argmin[r, n] == e ? Gmin[r, n] : 0)
 *                (evaluated left to right: t = Gsum; t = fma(2 p_e, Gsq, t); t += Gmax where e won; t += Gmin where e won)
 *     dB[c, n] = sum over the entries of column c of val[e] * t_e[n]   (fma; one GATHER pass over the rows of A^T)
 *     dval[e]  = sum_n B[c, n] * t_e[n]                                (fma; one row pass over A, one lane owns an entry)
 * N: a multiple of 8, at least 8, no upper limit but 65535 column tiles (see DESIGN 4.18 for this family's tile).  Leading dimensions:
 * ldb and lddb always, a struct member's when its pointer is given (ld_arg: when either arg is): >= N and multiples of 4; every pointer
 * 16-byte aligned.  The outputs must not overlap the inputs or each other.
 * d_val == NULL: the engine's current values.  No value refresh happens and none of the engine's packed forms is read or written.
 * Backward: d_dB or d_dval may be NULL, not both; d_B may be NULL when neither d_gsumsq nor d_dval is given.  It writes every element
 * of dB (K x N) and of dval (nnz) it is given.
 * First calls build the row softmax's tables / A^T as for sextans_spmm_reduce_device_rm and synchronise then; after that a call allocates
 * nothing, reads nothing back and does not synchronise: it can be captured into a hipGraph.
 * sextans_last_kernel: "spmm_multi" / "spmm_multi_backward", "+long_rows" appended when the workgroup path ran.
 * SEXTANS_ERR_INVALID: h == NULL, out / g == NULL, a bad N, a bad leading dimension, a misaligned pointer, no output (no gradient)
 * given, an arg without its value, (backward) d_gmax without d_argmax or d_gmin without d_argmin, d_dB and d_dval both NULL, d_gsumsq
 * or d_dval without d_B -- then the handle's state (SEXTANS_ERR_STATE: no CSR matrix set), then SEXTANS_ERR_INVALID for
 * nnz > INT32_MAX and (forward) d_B == NULL with nnz > 0; all before any device is touched.  M == 0 or nnz == 0: OK -- the values and
 * dB are zeroed, the args = -1. */
typedef struct { float *d_sum, *d_sumsq, *d_max, *d_min; int64_t ld_sum, ld_sumsq, ld_max, ld_min;
                 int32_t *d_argmax, *d_argmin; int64_t ld_arg; } sextans_multi_out;
typedef struct { const float *d_gsum, *d_gsumsq, *d_gmax, *d_gmin; int64_t ld_gsum, ld_gsumsq, ld_gmax, ld_gmin;
                 const int32_t *d_argmax, *d_argmin; int64_t ld_arg; } sextans_multi_grad;
int sextans_spmm_multi_device_rm(sextans_handle_t h, int N, const float *d_val, const float *d_B, int64_t ldb,
                                 const sextans_multi_out *out, void *stream);
int sextans_spmm_multi_backward_device_rm(sextans_handle_t h, int N, const float *d_val, const float *d_B, int64_t ldb,
                                          const sextans_multi_grad *g, float *d_dB, int64_t lddb, float *d_dval, void *stream);

/* ---- Softmax aggregation: a softmax PER OUTPUT COLUMN over a row's messages themselves, with a temperature per column (PyG's
 * SoftmaxAggregation(t, learn=True), the aggregator of GENConv / DeeperGCN, an entry of MultiAggregation).  It spans the mean (t = 0), the
 * max (t -> inf) and the min (t -> -inf).  Closest thing in the reference: none.
 *
 * A, B, d_val and the message p_e[n] = val[e] * B[c, n] (ONE rounded fp32 product) are those of sextans_spmm_reduce_device_rm above.  d_t: N
 * floats, one temperature per column, any finite value; NULL = 1.  All arithmetic fp32:
 *     s_e[n]    = t[n] * p_e[n]                   (one rounded multiply; d_t == NULL: s_e = p_e)
 *     lse[r, n] = log sum_e exp(s_e[n])           w_e[n] = exp(s_e[n] - lse[r, n])
 *     C[r, n]   = sum_e w_e[n] p_e[n]             a row without stored entries: C = +0, lse = -inf
 * computed online (a running maximum, normaliser and accumulator per (row, column); only differences to the maximum are exponentiated, so
 * t p beyond +-88 does not overflow), C = acc / z, lse = m + log z.  A row of ONE entry gives C the bits of its product (+0 for -0).  A
 * non-finite product does what this arithmetic makes of it (two infinite scores: NaN) within its own (row, column) and goes nowhere else.
 * Backward, G the upstream gradient of C, q_e[n] = (G[r, n] w_e[n]) (1 + t[n] (p_e[n] - C[r, n])):
 *     dB[c, n] = sum over the entries of column c of val[e] q_e[n]                  (fma; one GATHER pass over the rows of A^T)
 *     dval[e]  = sum_n B[c, n] q_e[n]                                               (fma; one row pass over A, one lane owns an entry)
 *     dt[n]    = sum_r sum_e (G[r, n] w_e[n]) (p_e[n] (p_e[n] - C[r, n]))           (the row pass leaves the inner sum per row in d_work;
 *                rows are then added in a fixed two-level order: 256-row chunks ascending, then the chunks ascending)
 * The gradients amplify the rounding of s by t (p - C): at |t| of a few hundred they lose digits that the forward keeps.
 * Every sum runs in an order fixed by the pattern and the launch shape; there are no atomics: the same bits on every run and stream.
 * Nothing of size nnz x N exists.  No value refresh happens and none of the engine's packed forms is read or written.
 * N: a multiple of 8, at least 8, no upper limit but 65535 column tiles of up to 128 floats.  Leading dimensions (all of them, whether or
 * not their pointer is NULL): >= N and multiples of 4; every pointer 16-byte aligned.  The outputs must not overlap the inputs or each other.
 * d_lse may be NULL in the forward (inference).  In the backward any of d_dB, d_dval, d_dt may be NULL, not all three; d_dt needs d_work,
 * sextans_spmm_softagg_workspace_floats(h, N) = M * N + ceil(M / 256) * N floats that the call writes (only when d_dt is given).  The
 * backward writes every element of dB (K x N), dval (nnz) and dt (N) it is given.
 * First calls build the row softmax's tables / A^T as for sextans_spmm_reduce_device_rm and synchronise then; after that a call allocates
 * nothing, reads nothing back and does not synchronise: it can be captured into a hipGraph.
 * sextans_last_kernel: "spmm_softagg" / "spmm_softagg_backward", "+long_rows" appended when the workgroup path ran.
 * SEXTANS_ERR_INVALID: h == NULL, N < 8 or not a multiple of 8, a leading dimension below N or not a multiple of 4, a misaligned pointer,
 * (backward) d_dB, d_dval and d_dt all NULL, d_dt without d_work -- checked in this order, then the handle's state (SEXTANS_ERR_STATE: no CSR
 * matrix set), then SEXTANS_ERR_INVALID for nnz > INT32_MAX and for a required pointer (B, C, and in the backward lse and G) that is NULL
 * with nnz > 0; all before any device is touched.  sextans_spmm_softagg_workspace_floats returns the error code negated.  M == 0 or
 * nnz == 0: OK -- C, dB, dt and the workspace are zeroed, lse = -inf. */
int sextans_spmm_softagg_device_rm(sextans_handle_t h, int N, const float *d_val, const float *d_B, int64_t ldb, const float *d_t,
                                   float *d_C, int64_t ldc, float *d_lse, int64_t ldlse, void *stream);
int64_t sextans_spmm_softagg_workspace_floats(sextans_handle_t h, int N);
int sextans_spmm_softagg_backward_device_rm(sextans_handle_t h, int N, const float *d_val, const float *d_B, int64_t ldb, const float *d_t,
                                            const float *d_C, int64_t ldc, const float *d_lse, int64_t ldlse, const float *d_G, int64_t ldg,
                                            float *d_dB, int64_t lddb, float *d_dval, float *d_dt, float *d_work, void *stream);

/* ---- SpMM with a feature VECTOR per stored entry (edge-feature message passing: continuous-filter convolution / u_mul_e_sum, GINE /
 * relu(u_add_e) summed, edge -> node reduction / copy_e_sum).  Closest thing in the reference: none -- its PEs weight an entry with a
 * scalar.
 *
 * Only the PATTERN of the engine's M x K CSR matrix is used: its values are neither read nor touched, and no value refresh happens.
 * B row-major K x N fp32 (B[k * ldb + n]), C and G row-major M x N, E and dE row-major nnz x N IN THE CSR ENTRY ORDER the matrix was set
 * with: E[e * lde + n] belongs to the entry at position e of the CSR arrays (offsets are 64-bit: nnz * N may exceed 2^31).
 * For the stored entry e = (r, c) and column n the message is ONE rounded fp32 operation, never fused with the sum:
 *     SEXTANS_EDGE_MUL       m = B[c, n] * E[e, n]
 *     SEXTANS_EDGE_ADD       m = B[c, n] + E[e, n]
 *     SEXTANS_EDGE_ADD_RELU  s = B[c, n] + E[e, n];  m = s > 0 ? s : (s != s ? s : +0)
 *     SEXTANS_EDGE_COPY      m = E[e, n]                    (d_B is not read and may be NULL)
 *     forward    C[r, n]  = sum over row r's entries of m   (fp32 adds rounded to nearest, in an order fixed by the pattern and the
 *                launch shape; a row without entries gives +0; NaN and +-inf reach the rows and columns whose entries hold them only)
 *     backward   dE[e, n] = G[r, n] * B[c, n] (MUL) | G[r, n] (ADD, COPY) | (B[c, n] + E[e, n] > 0 ? G[r, n] : +0) (ADD_RELU)
 *                -- one rounded operation per element: BIT-DETERMINED
 *                dB[c, n] = sum over the entries of column c of G[r, n] * E[e, n] (MUL, fused multiply-add) | G[r, n] (ADD) | the masked
 *                G[r, n] (ADD_RELU); a column without entries gives 0.  COPY has no dB.
 * There are no atomics anywhere: dB is a GATHER over the rows of A^T (sextans_csr_transpose_device's arrays and entry permutation), dE
 * a row pass in which one group of lanes owns an (entry, tile) and stores it.  The same call gives the same bits on every run and stream.
 * N: a multiple of 8, at least 8, no upper limit but 65535 tiles: the columns are cut into tiles of the smallest of 8 / 16 / 32 / 64 /
 * 128 floats that holds min(N, 128), which play the part the heads play in sextans_attention_device (per entry one 4-byte column load,
 * the 16-byte pieces of one gathered B row and of the entry's own E row; rows -- column pass: columns -- of more than 2048 entries get
 * one workgroup per tile, merged through LDS).  The last tile may be partial.  E is read once per pass, dE written once.
 * Leading dimensions: >= N, multiples of 4 (all of them, whether or not their pointer is NULL); every pointer 16-byte aligned.  The
 * outputs must not overlap the inputs or each other.
 * Backward: d_dB or d_dE may be NULL, not both; d_dB must be NULL with SEXTANS_EDGE_COPY.  Needed with nnz > 0: d_G always; MUL: d_E for
 * dB, d_B for dE; ADD_RELU: d_B and d_E; ADD and COPY: neither (NULL is accepted).  The backward writes every element of dB (K x N) and
 * of dE (nnz x N) it is given.
 * The first forward call on a matrix validates it and builds the row softmax's tables; the first backward call with d_dB also builds
 * A^T (its arrays and the companion engine's tables only); both synchronise then.  After that a call allocates nothing, reads nothing
 * back and does not synchronise: it can be captured into a hipGraph.
 * sextans_last_kernel: "spmm_edge" / "spmm_edge_backward", "+long_rows" appended when the workgroup path ran.
 * SEXTANS_ERR_INVALID: h == NULL, op not one of the four, N < 8 or not a multiple of 8 or more than 65535 tiles, a leading dimension
 * below N or not a multiple of 4, a misaligned pointer, (backward) d_dB and d_dE both NULL, d_dB with COPY -- then the handle's state
 * (SEXTANS_ERR_STATE: no CSR matrix set), then SEXTANS_ERR_INVALID for nnz > INT32_MAX and for a required pointer that is NULL with
 * nnz > 0; all before any device is touched.  M == 0 or nnz == 0: OK -- C and dB are zeroed, dE has no element. */
#define SEXTANS_EDGE_MUL 1
#define SEXTANS_EDGE_ADD 2
#define SEXTANS_EDGE_ADD_RELU 3
#define SEXTANS_EDGE_COPY 4
int sextans_spmm_edge_device_rm(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const float *d_E, int64_t lde,
                                float *d_C, int64_t ldc, void *stream);
int sextans_spmm_edge_backward_device_rm(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const float *d_E, int64_t lde,
                                         const float *d_G, int64_t ldg, float *d_dB, int64_t lddb, float *d_dE, int64_t ldde, void *stream);

/* ---- Several aggregations of EDGE-FEATURE messages in one pass: the messages of sextans_spmm_edge_device_rm under the aggregates of
 * sextans_spmm_multi_device_rm (PNAConv over an edge MLP's messages = COPY under mean / max / min / std; EdgeConv, DGCNN = copy_e_max;
 * DGL's u_mul_e_max and u_add_e_max; MultiAggregation over any materialised message).  Closest thing in the reference: none.
 *
 * Only the PATTERN of the engine's M x K CSR matrix is used.  B, E, op and the message m[e, n] (ONE rounded fp32 operation, the relu of
 * ADD_RELU keeping a NaN) are those of sextans_spmm_edge_device_rm above; the outputs, sextans_multi_out and sextans_multi_grad those of
 * sextans_spmm_multi_device_rm (own pointer and leading dimension each, so that they may be column slices of one (M, k N) buffer):
 *     d_sum      sum_e m                          (fp32 adds rounded to nearest)
 *     d_sumsq    sum_e m^2                        (s = fma(m, m, s))
 *     d_max / d_argmax, d_min / d_argmin           a NaN wins, then the better value, then the smaller entry position; the args are
 *                                                  positions in the CSR arrays (= rows of E)
 *     a row without stored entries: sums +0, max and min +0, args -1; a row of one entry: sum has the message's bits
 * The sums run in an order fixed by the pattern and the launch shape (no atomics: the same bits on every run and stream) that does not
 * depend on which outputs are requested.  A NULL output is not computed (the groups of sextans_spmm_multi_device_rm); at least one of
 * the four values must be given, and an arg needs its value.
 * Backward, for the upstream gradients that are given (NULL: absent) and the args of the forward:
 *     t_e[n]   = Gsum[r, n] + 2 m[e, n] Gsq[r, n] + (argmax[r, n] == e ? Gmax[r, n] : 0) + (argmin[r, n] == e ? Gmin[r, n] : 0)
 *                (evaluated left to right as for sextans_spmm_multi_backward_device_rm)
 *     dB[c, n] = sum over the entries of column c of E[e, n] * t_e[n] (MUL, fused multiply-add) | t_e[n] (ADD) |
 *                (B[c, n] + E[e, n] > 0 ? t_e[n] : 0) (ADD_RELU); COPY has no dB      (one GATHER pass over the rows of A^T)
 *     dE[e, n] = t_e[n] * B[c, n] (MUL) | t_e[n] (ADD, COPY) | (B[c, n] + E[e, n] > 0 ? t_e[n] : +0) (ADD_RELU)
 *                -- one rounded operation per element, stored once: BIT-DETERMINED (ADD / COPY with d_gsum alone: G's bits)
 * Nothing of size nnz x N exists besides E and dE.
 * N: a multiple of 8, at least 8, no upper limit but 65535 column tiles of up to 64 floats.  Leading dimensions: ldb, lde,
 * lddb and ldde always, a struct member's when its pointer is given (ld_arg: when either arg is): >= N and multiples of 4; every pointer
 * 16-byte aligned.  The outputs must not overlap the inputs or each other.
 * Needed with nnz > 0: d_E always; d_B unless op is SEXTANS_EDGE_COPY (then d_B may be NULL and d_dB must be).  The pointers are
 * required by rule; a kernel reads an operand only where its formula does.  Backward: d_dB or d_dE may be NULL, not both; it writes every
 * element of dB (K x N) and of dE (nnz x N) it is given.
 * First calls build the row softmax's tables / A^T as for sextans_spmm_edge_device_rm and synchronise then; after that a call allocates
 * nothing, reads nothing back and does not synchronise: it can be captured into a hipGraph.
 * sextans_last_kernel: "spmm_edge_multi" / "spmm_edge_multi_backward", "+long_rows" appended when the workgroup path ran.
 * SEXTANS_ERR_INVALID: h == NULL, out / g == NULL, op not one of the four, a bad N, a bad leading dimension, a misaligned pointer, no
 * output (no gradient) given, an arg without its value, (backward) d_gmax without d_argmax or d_gmin without d_argmin, d_dB and d_dE
 * both NULL, d_dB with COPY -- then the handle's state (SEXTANS_ERR_STATE: no CSR matrix set), then SEXTANS_ERR_INVALID for
 * nnz > INT32_MAX and for a required pointer that is NULL with nnz > 0; all before any device is touched.  M == 0 or nnz == 0: OK -- the
 * values and dB are zeroed, the args = -1, dE has no element. */
int sextans_spmm_edge_multi_device_rm(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const float *d_E, int64_t lde,
                                      const sextans_multi_out *out, void *stream);
int sextans_spmm_edge_multi_backward_device_rm(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const float *d_E, int64_t lde,
                                               const sextans_multi_grad *g, float *d_dB, int64_t lddb, float *d_dE, int64_t ldde, void *stream);

/* ---- Softmax aggregation of EDGE-FEATURE messages: the messages of sextans_spmm_edge_device_rm under the per-column softmax of
 * sextans_spmm_softagg_device_rm (GENConv / DeeperGCN on graphs with edge features, whose message is relu(x_j + e_ij) + eps: ADD_RELU;
 * PyG's SoftmaxAggregation over any materialised message: COPY).  Closest thing in the reference: none.
 *
 * Only the PATTERN of the engine's M x K CSR matrix is used: its values are neither read nor touched, and no value refresh happens.
 * B, E, op and the message m_e[n] (ONE rounded fp32 operation, the relu of ADD_RELU keeping a NaN) are those of
 * sextans_spmm_edge_device_rm above; d_t, C and lse those of sextans_spmm_softagg_device_rm.  All arithmetic fp32:
 *     s_e[n]    = t[n] * m_e[n]                   (one rounded multiply, never fused; d_t == NULL: s_e = m_e)
 *     lse[r, n] = log sum_e exp(s_e[n])           w_e[n] = exp(s_e[n] - lse[r, n])
 *     C[r, n]   = sum_e w_e[n] m_e[n]             a row without stored entries: C = +0, lse = -inf
 * computed online exactly as sextans_spmm_softagg_device_rm does (running maximum, normaliser and accumulator per (row, column); t m may be
 * anything finite): with SEXTANS_EDGE_MUL and E[e, :] = val[e] the call returns that function's bits for N <= 64.  A row of ONE entry gives
 * C the bits of its message (+0 for -0).  A non-finite message does what this arithmetic makes of it within its own (row, column) and goes
 * nowhere else.  A shift common to a row's messages (GENConv's + eps) cancels in the weights: add it to C on the rows that have entries.
 * Backward, G the upstream gradient of C, q_e[n] = (G[r, n] w_e[n]) fma(t[n], m_e[n] - C[r, n], 1)   (= dL/dm_e; all three passes
 * recompute m_e and s_e with the same operations, so they see the same bits):
 *     dE[e, n] = q_e[n] * B[c, n] (MUL) | q_e[n] (ADD, COPY) | (B[c, n] + E[e, n] > 0 ? q_e[n] : +0) (ADD_RELU)
 *                (one row pass over A; every element stored once by the lanes that own its (entry, tile))
 *     dt[n]    = sum_r G[r, n] sum_e w_e[n] m_e[n] (m_e[n] - C[r, n])   (the row pass leaves the inner sum per row in d_work; rows are then
 *                added in a fixed two-level order: 256-row chunks ascending, then the chunks ascending)
 *     dB[c, n] = sum over the entries of column c of q_e[n] * E[e, n] (MUL, fused multiply-add) | q_e[n] (ADD) |
 *                (B[c, n] + E[e, n] > 0 ? q_e[n] : 0) (ADD_RELU); COPY has no dB        (one GATHER pass over the rows of A^T)
 * The gradients amplify the rounding of s by t (m - C): at |t| of a few hundred they lose digits that the forward keeps.
 * Every sum runs in an order fixed by the pattern and the launch shape; there are no atomics: the same bits on every run and stream.
 * Nothing of size nnz x N exists besides E and dE.
 * N: a multiple of 8, at least 8, no upper limit but 65535 column tiles of up to 64 floats.  Leading dimensions: >= N and
 * multiples of 4 -- lde, ldc, ldg and (backward) ldlse always; ldb unless d_B is NULL with SEXTANS_EDGE_COPY; ldlse in the forward, lddb
 * and ldde when their pointer is given.  Every pointer 16-byte aligned.  The outputs must not overlap the inputs or each other.
 * Needed with nnz > 0: d_E and d_C always; d_B unless op is SEXTANS_EDGE_COPY (then d_B may be NULL and d_dB must be); in the backward
 * also d_lse and d_G.  d_lse may be NULL in the forward (inference).  In the backward any of d_dB, d_dE, d_dt may be NULL, not all three;
 * d_dt needs d_work, sextans_spmm_edge_softagg_workspace_floats(h, N) = M * N + ceil(M / 256) * N floats that the call writes (only when
 * d_dt is given).  The backward writes every element of dB (K x N), dE (nnz x N) and dt (N) it is given; the column pass runs only for
 * d_dB, the row pass for d_dE or d_dt.
 * The first forward call on a matrix validates it and builds the row softmax's tables; the first backward call with d_dB also builds A^T
 * (its arrays and the companion engine's tables only); both synchronise then.  After that a call allocates nothing, reads nothing back
 * and does not synchronise: it can be captured into a hipGraph.
 * sextans_last_kernel: "spmm_edge_softagg" / "spmm_edge_softagg_backward", "+long_rows" appended when the workgroup path ran.
 * SEXTANS_ERR_INVALID: h == NULL, op not one of the four, N < 8 or not a multiple of 8 or more than 65535 tiles, a leading dimension
 * below N or not a multiple of 4, a misaligned pointer, (backward) d_dB, d_dE and d_dt all NULL, d_dt without d_work, d_dB with COPY --
 * checked in this order, then the handle's state (SEXTANS_ERR_STATE: no CSR matrix set), then SEXTANS_ERR_INVALID for nnz > INT32_MAX
 * and for a required pointer that is NULL with nnz > 0; all before any device is touched.
 * sextans_spmm_edge_softagg_workspace_floats returns the error code negated.  M == 0 or nnz == 0: OK -- C, dB, dt and the workspace are
 * zeroed, lse = -inf, dE has no element. */
int sextans_spmm_edge_softagg_device_rm(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const float *d_E, int64_t lde,
                                        const float *d_t, float *d_C, int64_t ldc, float *d_lse, int64_t ldlse, void *stream);
int64_t sextans_spmm_edge_softagg_workspace_floats(sextans_handle_t h, int N);
int sextans_spmm_edge_softagg_backward_device_rm(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const float *d_E,
                                                 int64_t lde, const float *d_t, const float *d_C, int64_t ldc, const float *d_lse,
                                                 int64_t ldlse, const float *d_G, int64_t ldg, float *d_dB, int64_t lddb, float *d_dE,
                                                 int64_t ldde, float *d_dt, float *d_work, void *stream);

/* ---- Channel-wise ("vector") attention from caller-supplied PER-CHANNEL scores: the per-column softmax of
 * sextans_spmm_edge_softagg_device_rm with the score decoupled from the message (PointTransformerConv:
 * x_i' = sum_j softmax_j(gamma(phi(x_i) - psi(x_j) + delta_ij)) * (W x_j + delta_ij), the score an (nnz, N) tensor out of an MLP; DGL's
 * edge_softmax on multi-channel edge data followed by u_mul_e_sum / e_mul_e; PyG's softmax(alpha, index) with a per-channel alpha;
 * AttentionalAggregation with a per-channel gate).  Closest thing in the reference: none.
 *
 * Only the PATTERN of the engine's M x K CSR matrix is used: its values are neither read nor touched, and no value refresh happens.
 * S, D, dS and dD are (nnz, N) row-major IN THE CSR ENTRY ORDER (element [e * ld + n], 64-bit offsets); V and dV are (K, N); C, lse and G
 * are (M, N).  For the stored entry e = (r, c) and column n, all arithmetic fp32:
 *     SEXTANS_VATT_NODE   m_e = V[c, n]                 (d_D is ignored)
 *     SEXTANS_VATT_ADD    m_e = V[c, n] + D[e, n]       (ONE rounded add)
 *     SEXTANS_VATT_EDGE   m_e = D[e, n]                 (d_V is ignored)
 *     s_e = S[e, n]                                     (read, never computed)
 *     lse[r, n] = log sum_e exp(s_e)      w_e = exp(s_e - lse[r, n])      C[r, n] = sum_e w_e m_e
 * computed online exactly as sextans_spmm_edge_softagg_device_rm does (running maximum, normaliser and accumulator per (row, column); the
 * scores may be anything finite): fed S = t[n] m_e formed as one rounded product, ADD and EDGE return the bits of that function's ADD
 * and COPY and NODE those of sextans_spmm_softagg_device_rm on values of 1, for N <= 64.  A row without stored entries: C = +0,
 * lse = -inf.  A row of ONE entry gives C the bits of its message (+0 for -0) and lse = s.  A score of -inf MASKS its (entry, column): the
 * weight is exactly +0 and dS is +0 there; a (row, column) whose scores are all -inf ends as 0 / 0: C is NaN there, lse -inf, and the NaN
 * stays in that (row, column).  Any other non-finite score or message stays in its own (row, column) as well.
 * Backward, G the upstream gradient of C, gw_e = G[r, n] w_e (both passes recompute w_e with the same operations: the same bits):
 *     dS[e, n] = gw_e (m_e - C[r, n])   (+0 where S[e, n] = -inf)       dD[e, n] = gw_e   (ADD, EDGE)
 *                (one row pass over A; every element stored once by the lanes that own its (entry, tile))
 *     dV[c, n] = sum over the entries of column c of gw_e   (NODE, ADD)      (one GATHER pass over the rows of A^T, which reads S through
 *                the transpose's permutation and gathers lse and G; neither C, V nor D)
 * Every sum runs in an order fixed by the pattern and the launch shape; there are no atomics: the same bits on every run and stream.
 * N: a multiple of 8, at least 8, no upper limit but 65535 column tiles of up to 64 floats.  Leading dimensions: >= N and
 * multiples of 4 -- lds, ldc, ldg and (backward) ldlse always; ldv unless msg is EDGE, ldd unless msg is NODE; ldlse in the forward,
 * ldds, lddv and lddd when their pointer is given.  Every pointer that is read or written 16-byte aligned.  An operand the mode does not
 * read (d_V with EDGE, d_D with NODE) is ignored with its leading dimension.  The outputs must not overlap the inputs or each other; in
 * ADD mode dS and dD are two distinct buffers.
 * Needed with nnz > 0: d_S, d_C and the operands the mode reads; in the backward also d_lse and d_G.  d_lse may be NULL in the forward
 * (inference).  In the backward any of d_dS, d_dV, d_dD may be NULL, not all three; the row pass runs when d_dS or d_dD is given, the
 * column pass when d_dV is given; every element of a gradient that is given is written.
 * The first forward call on a matrix validates it and builds the row softmax's tables; the first backward call with d_dV also builds A^T
 * (its arrays and the companion engine's tables only); both synchronise then.  After that a call allocates nothing, reads nothing back
 * and does not synchronise: it can be captured into a hipGraph.  The caller's stream is used.
 * sextans_last_kernel: "vector_attention" / "vector_attention_backward", "+long_rows" appended when the workgroup path ran.
 * SEXTANS_ERR_INVALID: h == NULL, msg not one of the three, N < 8 or not a multiple of 8 or more than 65535 tiles, a leading dimension
 * below N or not a multiple of 4, a misaligned pointer, (backward) d_dS, d_dV and d_dD all NULL, d_dV with EDGE, d_dD with NODE --
 * checked in this order, then the handle's state (SEXTANS_ERR_STATE: no CSR matrix set), then SEXTANS_ERR_INVALID for nnz > INT32_MAX
 * and for a required pointer that is NULL with nnz > 0; all before any device is touched.  M == 0 or nnz == 0: OK -- C and dV are
 * zeroed, lse = -inf, dS and dD have no element. */
#define SEXTANS_VATT_NODE 1
#define SEXTANS_VATT_ADD 2
#define SEXTANS_VATT_EDGE 3
int sextans_vector_attention_device_rm(sextans_handle_t h, int msg, int N, const float *d_S, int64_t lds, const float *d_V, int64_t ldv,
                                       const float *d_D, int64_t ldd, float *d_C, int64_t ldc, float *d_lse, int64_t ldlse, void *stream);
int sextans_vector_attention_backward_device_rm(sextans_handle_t h, int msg, int N, const float *d_S, int64_t lds, const float *d_V, int64_t ldv,
                                                const float *d_D, int64_t ldd, const float *d_C, int64_t ldc, const float *d_lse, int64_t ldlse,
                                                const float *d_G, int64_t ldg, float *d_dS, int64_t ldds, float *d_dV, int64_t lddv,
                                                float *d_dD, int64_t lddd, void *stream);

/* ---- Edge-OUTPUT ops from both endpoints of every stored entry (DGL's gSDDMM next to gSpMM: u_add_v, u_sub_v, u_mul_v, copy_u, copy_v,
 * each optionally + e): the (nnz, N) tensors that sextans_score_attention_device, sextans_vector_attention_device_rm,
 * sextans_spmm_edge*_device_rm and sextans_spmm_edge_softagg_device_rm READ -- Point Transformer's phi(x_i) - psi(x_j) + delta_ij,
 * EdgeConv's x_j - x_i, the halves of MeshGraphNets' concat(e, x_i, x_j) (ldz places them), the argument of an MLP on x_i * x_j, GatedGCN's
 * pre-activations without the aggregation -- without two materialised gathers and without an atomic scatter in the backward.  Closest
 * thing in the reference: none.
 *
 * Only the PATTERN of the engine's M x K CSR matrix is used: its values are neither read nor touched, and no value refresh happens.
 * xdst and dxdst are row-major M x N fp32, xsrc and dxsrc K x N; Z, E and Gz are (nnz, N) row-major IN THE CSR ENTRY ORDER the matrix was
 * set with, as E of sextans_spmm_edge_device_rm (element [e * ld + n], 64-bit offsets).  For the stored entry e = (r, c) and column n
 * every result is ONE rounded fp32 operation:
 *     SEXTANS_EDGEOP_ADD   z = xdst[r, n] + xsrc[c, n]
 *     SEXTANS_EDGEOP_SUB   z = xdst[r, n] - xsrc[c, n]
 *     SEXTANS_EDGEOP_MUL   z = xdst[r, n] * xsrc[c, n]
 *     SEXTANS_EDGEOP_DST   z = xdst[r, n]                 (d_xsrc is ignored)
 *     SEXTANS_EDGEOP_SRC   z = xsrc[c, n]                 (d_xdst is ignored)
 *     Z[e, n] = z                  when d_E == NULL
 *     Z[e, n] = z + E[e, n]        otherwise: a second rounded add, in this order, never contracted
 * The forward is bit-determined: the bits of the same float32 expression anywhere.  MUL returns the bits of
 * sextans_spmm_edge_backward_device_rm's dE (G := xdst, B := xsrc), ADD with E those of sextans_spmm_gated_device_rm's z.
 * Backward, Gz the upstream gradient of Z (dE = Gz: no kernel and no argument):
 *     dxdst[r, n] = sum over row r's entries of Gz[e, n] (ADD, SUB, DST) | fma(Gz[e, n], xsrc[c, n], .) (MUL)
 *                   (one pass over the rows of A)
 *     dxsrc[c, n] = sum over column c's entries of Gz[e, n] (ADD, SRC) | fma(Gz[e, n], xdst[r, n], .) (MUL); SUB subtracts Gz[e, n] from an
 *                   accumulator that starts at +0: ADD's bits negated, except that a zero sum is +0
 *                   (the same pass over the rows of A^T, which reads Gz through the transpose's permutation)
 * d_dxdst or d_dxsrc may be NULL, not both: its pass is skipped, and with d_dxsrc == NULL A^T is never built.  The backward reads xsrc
 * only for MUL's dxdst and xdst only for MUL's dxsrc; otherwise they are ignored with their leading dimensions.  No atomics, no
 * workspace, no value refresh; every sum runs in an order fixed by the pattern and the launch shape: the same bits on every run and
 * stream.  Everything handed in is written in full: a row or column without entries gets +0.  NaN and +-inf reach only the entries,
 * rows and columns that hold them.
 * N: a multiple of 8, at least 8, no upper limit but 65535 column tiles of up to 128 floats.  Leading dimensions: >= N and
 * multiples of 4 -- ldz and ldgz always, those of the operands a call reads, lde, lddxdst and lddxsrc when their pointer is given.  Every
 * pointer that is read or written 16-byte aligned.  An operand the op does not read is ignored together with its leading dimension and
 * alignment.  The outputs must not overlap the inputs or each other; ldz > N writes Z into a wider buffer (a concatenation).
 * Needed with nnz > 0: d_Z, d_Gz and the operands the call reads.
 * The first forward call on a matrix validates it and builds the row softmax's tables; the first backward call with d_dxsrc also builds
 * A^T (its arrays and the companion engine's tables only); both synchronise then.  After that -- in particular after
 * sextans_prepare(h, N, SEXTANS_LAYOUT_ROWMAJOR_T, stream) -- a call allocates nothing, reads nothing back and does not synchronise: it
 * can be captured into a hipGraph.  The caller's stream is used.
 * sextans_last_kernel: "edge_op" / "edge_op_backward", "+long_rows" appended when the workgroup path ran.
 * SEXTANS_ERR_INVALID: h == NULL, op not one of the five, N < 8 or not a multiple of 8 or more than 65535 tiles, a leading dimension
 * below N or not a multiple of 4, a misaligned pointer, (backward) d_dxdst and d_dxsrc both NULL, d_dxdst with SRC, d_dxsrc with DST --
 * checked in this order, then the handle's state (SEXTANS_ERR_STATE: no CSR matrix set), then SEXTANS_ERR_INVALID for nnz > INT32_MAX
 * and for a required pointer that is NULL with nnz > 0; all before any device is touched.  M == 0 or nnz == 0: OK -- Z has no element,
 * dxdst and dxsrc are zeroed. */
#define SEXTANS_EDGEOP_ADD 1
#define SEXTANS_EDGEOP_SUB 2
#define SEXTANS_EDGEOP_MUL 3
#define SEXTANS_EDGEOP_DST 4
#define SEXTANS_EDGEOP_SRC 5
int sextans_edge_op_device_rm(sextans_handle_t h, int op, int N, const float *d_xdst, int64_t ldxdst, const float *d_xsrc, int64_t ldxsrc,
                              const float *d_E, int64_t lde, float *d_Z, int64_t ldz, void *stream);
int sextans_edge_op_backward_device_rm(sextans_handle_t h, int op, int N, const float *d_xdst, int64_t ldxdst, const float *d_xsrc,
                                       int64_t ldxsrc, const float *d_Gz, int64_t ldgz, float *d_dxdst, int64_t lddxdst, float *d_dxsrc,
                                       int64_t lddxsrc, void *stream);

/* ---- Per-head dot product of both endpoints of every stored entry (DGL's u_dot_v, the last member of its gSDDMM set): the (nnz, heads)
 * scores that sextans_score_attention_device reads -- AGNN's cosine score, HGT's K W Q, SuperGAT's dot-product mode, any clamped,
 * tempered or MLP-adjusted transformer score written as u_dot_v, elementwise ops, score_attention -- in ONE launch for all heads, without
 * gathered (nnz, heads, d) temporaries and without an atomic scatter in the backward.  Closest thing in the reference: none.
 *
 * Only the PATTERN of the engine's M x K CSR matrix is used: its values are neither read nor touched, and no value refresh happens.
 * X and dX are row-major M x heads*d fp32 (head h of row r at [r * ld + h * d]), Y and dY K x heads*d -- the operands of
 * sextans_score_attention_device; S and Gs are (nnz, heads) row-major IN THE CSR ENTRY ORDER the matrix was set with (element
 * [e * ld + h], 64-bit offsets).  For the stored entry e = (r, c) and head h:
 *     acc = +0;  acc = acc + X[r, h, n] * Y[c, h, n]  for n = 0 .. d-1 in this order;  S[e, h] = acc
 * every product and every sum rounded to fp32, never contracted, the same in STRICT and FAST: bit for bit a sequential float32 loop, and
 * bit for bit what sextans_sddmm_device_rm(h, d, 1.0f, X + h * d, ldx, Y + h * d, ldy, 0, NULL, out, ...) writes for head h.  There is
 * no alpha: a scale belongs on X or on S.  The work is dealt by non-zeros (a wavefront owns 256 consecutive entries whatever rows they
 * belong to), so a hub row spreads over hundreds of wavefronts.
 * Backward, Gs the upstream gradient of S:
 *     dX[r, h, :] = sum over row r's entries of Gs[e, h] * Y[c, h, :]       the bits of sextans_score_attention_device(SEXTANS_SCORE_WEIGHT)'s
 *                                                                           O with S := Gs, V := Y (one pass over the rows of A)
 *     dY[c, h, :] = sum over column c's entries of Gs[e, h] * X[r, h, :]    the bits of sextans_score_attention_backward_device(
 *                                                                           SEXTANS_SCORE_WEIGHT)'s dV with S := Gs, G := X (the rows of A^T)
 * d_dX or d_dY may be NULL, not both: its pass is skipped, and with d_dY == NULL A^T is never built.  The backward reads X only for dY
 * and Y only for dX; otherwise they are ignored with their leading dimensions.  No atomics, no workspace, no value refresh: the same
 * bits on every run and stream.  Everything handed in is written in full: a row or column without entries gets +0.  NaN and +-inf
 * reach only the entries, rows and columns that hold them.
 * heads: 1 .. 65535.  d: a multiple of 8 in [8, 128].  ldx, ldy, lddx, lddy: >= heads * d and multiples of 4 (those of the operands a
 * call reads or writes); lds, ldgs: >= heads (lds == heads: S leaves as 16-byte stores; wider: one store per element, the columns
 * beyond heads are left alone).  Every pointer that is read or written 16-byte aligned.  The outputs must not overlap the inputs or each
 * other.  Needed with nnz > 0: d_S, d_Gs and the operands the call reads.
 * The first forward call on a matrix validates it and builds the table of the 256-entry ranges' first rows; the first backward call
 * builds the row softmax's tables and, with d_dY, A^T; both synchronise then.  After sextans_prepare(h, N, SEXTANS_LAYOUT_ROWMAJOR_T,
 * stream) a call allocates nothing, reads nothing back and does not synchronise: it can be captured into a hipGraph.  The caller's
 * stream is used.
 * sextans_last_kernel: "edge_dot" / "edge_dot_backward", the latter with "+long_rows" appended when a pass ran the workgroup path.
 * SEXTANS_ERR_INVALID: h == NULL, heads < 1 or > 65535, d not a multiple of 8 in [8, 128], a leading dimension too small or (ldx, ldy,
 * lddx, lddy) not a multiple of 4, a misaligned pointer, (backward) d_dX and d_dY both NULL -- checked in this order, then the handle's
 * state (SEXTANS_ERR_STATE: no CSR matrix set), then SEXTANS_ERR_INVALID for nnz > INT32_MAX and for a required pointer that is NULL
 * with nnz > 0; all before any device is touched.  M == 0 or nnz == 0: OK -- S has no element, dX and dY are zeroed. */
int sextans_edge_dot_device(sextans_handle_t h, int heads, int d, const float *d_X, int64_t ldx, const float *d_Y, int64_t ldy, float *d_S,
                            int64_t lds, void *stream);
int sextans_edge_dot_backward_device(sextans_handle_t h, int heads, int d, const float *d_X, int64_t ldx, const float *d_Y, int64_t ldy,
                                     const float *d_Gs, int64_t ldgs, float *d_dX, int64_t lddx, float *d_dY, int64_t lddy, void *stream);

/* ---- Gated aggregation: a per-channel sigmoid gate on every stored entry, computed from both endpoints and, optionally, the entry's own
 * features (PyG's ResGatedGraphConv; GatedGCN of Bresson & Laurent, the MPNN of GraphGPS and of the LRGB / "Benchmarking GNNs" suites).
 * Closest thing in the reference: none.
 *
 * Only the PATTERN of the engine's M x K CSR matrix is used: its values are neither read nor touched, and no value refresh happens.
 * xdst is row-major M x N fp32, xsrc and V K x N, E (optional: d_e == NULL) nnz x N IN THE CSR ENTRY ORDER the matrix was set with, as E of
 * sextans_spmm_edge_device_rm (64-bit offsets).  For the stored entry e = (r, c) and column n, all arithmetic fp32:
 *     z_e[n]   = (xdst[r, n] + xsrc[c, n]) + E[e, n]       two rounded adds in this order; without E the first one alone
 *     g_e[n]   = 1 / (1 + exp(-z_e[n]))                    the division rounded to nearest: exactly 1 for large z, exactly +0 for very
 *                                                          negative z (z = +-200 included), never inf; a NaN stays a NaN
 *     num[r,n] = sum_e fma(g_e[n], V[c, n], num)           den[r, n] = sum_e g_e[n]          (partial sums merged by rounded adds)
 *     SEXTANS_GATE_SUM    C[r, n] = num[r, n]                              (ResGatedGraphConv)
 *     SEXTANS_GATE_NORM   C[r, n] = num[r, n] / (den[r, n] + eps)          (GatedGCN; one rounded add, one rounded division)
 *     a row without stored entries: C = +0 and den = +0 in either mode
 * d_den (optional) receives den (M x N) in either mode; d_z (optional) receives z (nnz x N, in the entry order, one plain store per
 * element): the layer's new edge features.  Without d_z nothing of size nnz x N is written, without d_e none is read.
 * Backward, G the upstream gradient of C and Gz (optional) that of z; gn = G (SUM) or G / (den + eps) (NORM), C read as 0 in SUM:
 *     dg_e[n]  = gn[r, n] (V[c, n] - C[r, n])              dz_e[n] = fma(dg_e[n], g_e[n] (1 - g_e[n]), Gz[e, n])
 *     dxdst[r, n] = sum_e dz_e[n]      dE[e, n] = dz_e[n]  (one store per element)                       -- a row pass over A
 *     dxsrc[c, n] = sum over the entries of column c of dz_e[n]      dV[c, n] = sum of fma(g_e[n], gn[r, n], dV)   -- a GATHER pass over A^T
 * z and g are RECOMPUTED with the forward's expressions (the same bits), not stored.  In NORM mode a small elementwise kernel writes gn
 * once into d_work, sextans_spmm_gated_workspace_floats(h, mode, N) floats (NORM: M * N; SUM: 0, d_work is not read and may be NULL);
 * both passes read it.  The row pass runs only when d_dxdst or d_de is given, the column pass (and with it A^T) only when d_dxsrc or
 * d_dv is; a gradient has the same bits whichever others are asked for.  d_de without d_e is allowed: the gradient of z.
 * There are no atomics anywhere; every sum runs in an order fixed by the pattern and the launch shape: the same bits on every run and stream.
 * N: a multiple of 8, at least 8, no upper limit but 65535 column tiles of up to 64 floats.  Leading dimensions: ld_xdst,
 * ld_xsrc, ld_v, ldc (forward) and ldg always, every other one when its pointer is given: >= N and multiples of 4; every pointer 16-byte
 * aligned.  The outputs must not overlap the inputs or each other.
 * eps: finite and > 0 in NORM mode; ignored in SUM mode.  d_C and d_den of the backward: required in NORM mode, ignored in SUM mode.
 * The backward writes every element of the gradients it is given (dxdst M x N, dxsrc and dV K x N, dE nnz x N).
 * First calls build the row softmax's tables / A^T as for sextans_spmm_edge_device_rm and synchronise then; after that a call allocates
 * nothing, reads nothing back and does not synchronise: it can be captured into a hipGraph.
 * sextans_last_kernel: "spmm_gated" / "spmm_gated_backward", "+long_rows" appended when the workgroup path ran.
 * SEXTANS_ERR_INVALID: h == NULL, in / out == NULL, mode not one of the two, a bad eps in NORM mode, a bad N, a bad leading dimension, a
 * misaligned pointer, (backward) no gradient pointer given -- then the handle's state (SEXTANS_ERR_STATE: no CSR matrix set), then
 * SEXTANS_ERR_INVALID for nnz > INT32_MAX and for a required pointer (xdst, xsrc, V, C; backward: G and, in NORM mode, C, den and d_work)
 * that is NULL with nnz > 0; all before any device is touched.  sextans_spmm_gated_workspace_floats returns the error code negated.
 * M == 0 or nnz == 0: OK -- C, den, dxdst, dxsrc and dV are zeroed; z and dE have no element. */
#define SEXTANS_GATE_SUM 1
#define SEXTANS_GATE_NORM 2
typedef struct { const float *d_xdst, *d_xsrc, *d_v, *d_e; int64_t ld_xdst, ld_xsrc, ld_v, ld_e; } sextans_gated_in;     /* d_e may be NULL */
typedef struct { float *d_dxdst, *d_dxsrc, *d_dv, *d_de; int64_t ld_dxdst, ld_dxsrc, ld_dv, ld_de; } sextans_gated_grad; /* any subset, not none */
int sextans_spmm_gated_device_rm(sextans_handle_t h, int mode, float eps, int N, const sextans_gated_in *in,
                                 float *d_C, int64_t ldc, float *d_den, int64_t ldden, float *d_z, int64_t ldz, void *stream);
int64_t sextans_spmm_gated_workspace_floats(sextans_handle_t h, int mode, int N);
int sextans_spmm_gated_backward_device_rm(sextans_handle_t h, int mode, float eps, int N, const sextans_gated_in *in,
                                          const float *d_C, int64_t ldc, const float *d_den, int64_t ldden,
                                          const float *d_G, int64_t ldg, const float *d_Gz, int64_t ldgz,
                                          const sextans_gated_grad *out, float *d_work, void *stream);

/* ---- Edge features inside the fused attention: a key row and a value row per stored entry (PyG's TransformerConv(edge_dim=...), UniMP,
 * the Dwivedi-Bresson graph transformer, relative-position encodings of mesh transformers).  Closest thing in the reference: none.
 *
 * Ek is (nnz, heads * d) and Ev (nnz, heads * dv), row-major in the entry order of the CSR arrays the matrix was set with
 * (Ek[e * ldek + h * d + i], 64-bit offsets), as E of sextans_spmm_edge_device_rm.  For the stored entry e = (r, c) and head h
 *     k_e = K[c,h,:] + Ek[e,h,:]       s_e = scale * (<Q[r,h,:], k_e> + bias_e)
 *     v_e = V[c,h,:] + Ev[e,h,:]       O[r,h,:] = sum_e softmax_e(s) v_e          lse[r,h] as in sextans_attention_device
 *     backward   dQ[r,h,:] = sum_e scale ds_e k_e;  dK[c,h,:] = sum_e scale ds_e Q[r,h,:];  dV[c,h,:] = sum_e (m_e p_e) G[r,h,:]
 *                dEk[e,h,:] = (scale ds_e) * Q[r,h,:];  dEv[e,h,:] = (m_e p_e) * G[r,h,:]   -- one rounded multiply per element
 *                with ds_e = p_e * (m_e <G[r,h,:], v_e> - delta[r,h]) and m_e the dropout multiplier (1 without dropout)
 * k_e and v_e are ONE rounded fp32 add per element, formed once per pass; everything after is the arithmetic of
 * sextans_attention_device (sextans_attention_dropout_device with drop) on k_e, v_e: the same row walking, lane groups, long-row
 * workgroups, merges and order of every sum, so all three passes recompute the same score bits.  Per (entry, head) the forward and the
 * row pass read one more 16-byte-piece row of each E given; the column pass (over A^T) reads both E a second time, through the
 * transpose's entry permutation.  An (entry, head) belongs to one group of lanes in the row pass, which stores its dEk and dEv pieces:
 * no atomics, no read-modify-write, the same bits on every run and stream; nothing of size nnz exists besides E, dE and the bias.
 * d_Ek or d_Ev may be NULL: that side has no edge term (k_e = K[c] / v_e = V[c], bit for bit).  Both NULL: the call IS
 * sextans_attention_dropout_device / _backward_device -- the plain kernels, the plain bits, their sextans_last_kernel.
 * drop == NULL or p == 0: no dropout, as there.
 * Backward: d_dEk and d_dEv may each be NULL (gradient not wanted).  d_dEk == d_dEv (one projected edge_attr used for both sides,
 * as PyG does): the sum dEk + dEv (one rounded add of the two pieces) is stored once -- needs both E, d == dv and lddek == lddev.
 * Leading dimensions: ldek, lddek >= heads * d, ldev, lddev >= heads * dv, multiples of 4, checked whether or not their pointer is
 * NULL; every pointer 16-byte aligned.  The outputs must not overlap the inputs or each other (but for d_dEk == d_dEv).
 * sextans_last_kernel: "attention_edge_fused" / "attention_edge_fused_backward", then "+dropout", then "+long_rows".
 * SEXTANS_ERR_INVALID: everything sextans_attention_dropout_device rejects, in its order, with the E leading dimensions and pointers
 * among the others; (backward) a gradient pointer for an absent E; d_dEk == d_dEv unless both E are given, d == dv and
 * lddek == lddev -- then SEXTANS_ERR_STATE for a handle without a CSR matrix, then SEXTANS_ERR_INVALID for nnz > INT32_MAX and for a
 * required pointer that is NULL with nnz > 0; all before any device is touched.  M == 0 or nnz == 0: OK -- O, delta, dQ, dK, dV are
 * zeroed, lse is -inf, dEk and dEv have no element. */
int sextans_attention_edge_device(sextans_handle_t h, int heads, int d, int dv, float scale,
    const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk, const float *d_V, int64_t ldv,
    const float *d_Ek, int64_t ldek, const float *d_Ev, int64_t ldev,
    const float *d_bias, float *d_O, int64_t ldo, float *d_lse, const sextans_dropout *drop, void *stream);
int sextans_attention_edge_backward_device(sextans_handle_t h, int heads, int d, int dv, float scale,
    const float *d_Q, int64_t ldq, const float *d_K, int64_t ldk, const float *d_V, int64_t ldv,
    const float *d_Ek, int64_t ldek, const float *d_Ev, int64_t ldev,
    const float *d_bias, const float *d_O, int64_t ldo, const float *d_lse, const float *d_G, int64_t ldg,
    float *d_delta, float *d_dQ, int64_t lddq, float *d_dK, int64_t lddk, float *d_dV, int64_t lddv,
    float *d_dEk, int64_t lddek, float *d_dEv, int64_t lddev, float *d_dbias, const sextans_dropout *drop, void *stream);

/* ---- Attention from caller-supplied per-head scores ("score attention"): the softmax of, or the plain weighting by, an (nnz, heads)
 * tensor S, times V, per head -- DGL's edge_softmax + u_mul_e_sum, PyG's softmax(alpha, index) + propagate; the piece HGT's typed
 * projections, AGNN's cosine score, SuperGAT, distance / RBF scores, a Graphormer-style per-head bias, an MLP on edge features or
 * coefficients kept from another layer are written with.  Closest thing in the reference: none.
 *
 * S and dS are (nnz, heads) row-major in the entry order of the CSR arrays the matrix was set with: element (e, h) is S[e * lds + h]
 * (64-bit offsets), read and written one float at a time, so lds, ldds >= heads is the only condition on them (as ldadst).  V, O, G, dV
 * as in sextans_gat_attention_device; lse is M x heads, dense.  A's own values are neither read nor written.  For the stored entry
 * e = (r, c), head h and m_e the dropout multiplier (1 without dropout):
 *   SEXTANS_SCORE_SOFTMAX   s_e = S[e,h];  O[r,h,:] = sum_e softmax_e(s) m_e V[c,h,:];  lse[r,h] = m + log Z
 *       the arithmetic of sextans_gat_attention_device from s onward (online softmax, exp2-based exp, FMA accumulation, dropped entries
 *       count in Z): fed the scores GAT computes, O, lse and dV are GAT's bits.
 *       backward   delta = <O[r,h,:], G[r,h,:]> (in registers: no workspace);  p_e = exp(s_e - lse[r,h])
 *                  dS[e,h] = p_e * (m_e <G[r,h,:], V[c,h,:]> - delta);  dV[c,h,:] = sum_e (m_e p_e) G[r,h,:]
 *   SEXTANS_SCORE_WEIGHT    O[r,h,:] = sum_e S[e,h] V[c,h,:], FMA in the slot's entry order.  d_lse is neither read nor written, forward
 *       and backward, and d_O not in the backward: they may be NULL there (and the backward does not look at ldo).
 *       backward   dS[e,h] = <G[r,h,:], V[c,h,:]>;  dV[c,h,:] = sum_e S[e,h] G[r,h,:]
 *       drop must be NULL or have p == 0: the caller holds the weights and can drop them.
 * The forward and the row pass run over A: one 4-byte load and one gathered V row per (entry, head); the row pass stores dS[e,h] from
 * one lane of the one group of lanes that owns the entry -- one plain store per element.  The column pass runs over A^T, reads
 * S[perm e, h] and lse[r,h], gathers G[r,h,:] and writes dV.  d_dS or d_dV may be NULL (not both): that pass is skipped, the other's
 * bits are unchanged.  Everything written is written in full: rows / columns without entries get +0, their lse -inf.  No atomics, the
 * same bits on every run and stream, nothing allocated beyond the softmax tables and A^T (after
 * sextans_prepare(h, N, SEXTANS_LAYOUT_ROWMAJOR_T, stream) the calls can be captured).
 * Special values (SOFTMAX): a -inf score is a mask and contributes exactly 0 everywhere; a row of only -inf scores, or with a +inf or
 * NaN score, gives NaN in that (row, head).  dv: a multiple of 8 in [8, 128]; ldv, ldo, ldg, lddv >= heads * dv, multiples of 4; every
 * pointer 16-byte aligned.  The outputs must not overlap the inputs or each other.
 * sextans_last_kernel: "score_softmax_fused" / "score_weight_fused", "..._backward", then "+dropout", then "+long_rows".
 * SEXTANS_ERR_INVALID, in this order: a NULL handle, a mode that is neither, heads < 1, a bad dv; a bad dropout (p outside [0, 1)) and
 * p > 0 in SEXTANS_SCORE_WEIGHT; the leading dimensions; alignment -- then SEXTANS_ERR_STATE for a handle without a CSR matrix, then
 * SEXTANS_ERR_INVALID for d_dS and d_dV both NULL and for a required pointer that is NULL with nnz > 0; all before any device is
 * touched.  M == 0 or nnz == 0: OK -- O and dV are zeroed, lse is -inf, dS has no element. */
#define SEXTANS_SCORE_SOFTMAX 1
#define SEXTANS_SCORE_WEIGHT 2
int sextans_score_attention_device(sextans_handle_t h, int mode, int heads, int dv,
    const float *d_S, int64_t lds, const float *d_V, int64_t ldv,
    float *d_O, int64_t ldo, float *d_lse, const sextans_dropout *drop, void *stream);
int sextans_score_attention_backward_device(sextans_handle_t h, int mode, int heads, int dv,
    const float *d_S, int64_t lds, const float *d_V, int64_t ldv,
    const float *d_O, int64_t ldo, const float *d_lse, const float *d_G, int64_t ldg,
    float *d_dS, int64_t ldds, float *d_dV, int64_t lddv, const sextans_dropout *drop, void *stream);

/* ---- bf16 DENSE operands on the row-major CSR entry (autocast activations, bf16 feature matrices).
 *
 * C = alpha * A * B + beta * C_in with B in bf16 (16-bit patterns, B[k * ldb + n]) and C_in / C_out BOTH of c_dtype: fp32 (float *) or
 * bf16 (uint16_t *).  A's values, every product and every sum stay fp32.  ld are in ELEMENTS, ldb, ldc_in, ldc >= N, N % 8 == 0; C_in may
 * alias C_out (same dtype).  With b32 = B widened to fp32 (exact: 16 zero bits appended) and c32 = C_in widened (or itself):
 *   the fp32 result is BIT FOR BIT what sextans_spmm_device_rm(h, N, alpha, b32, ..., beta, c32, ...) writes on the same engine with the
 *   same options -- in SEXTANS_MODE_STRICT bit-identical to cpu_spmm_CSR on b32, in SEXTANS_MODE_FAST inside that mode's stated bound;
 *   a bf16 C_out is that fp32 result rounded to nearest even (a NaN stays a NaN).
 * Route: the decision of sextans_spmm_device_rm for the call is taken unchanged.
 *   NATIVE   where it is the gather kernel (sextans_last_kernel "spmm_csr_rowgroup_rowmajor[+long_rows]" on the fp32 entry), no row is an
 *            exact chain (stat "exact_chain_rows" == 0) and the operands allow 16-byte accesses (16-byte aligned pointers, ldb % 8 == 0,
 *            C's ld % 4 == 0 for fp32 / % 8 == 0 for bf16; B below 4 GB: K * ldb * 2 < 2^32): the bf16 kernels (spmm_bf16_kernels.h) run on the caller's buffers -- one
 *            16-byte request per non-zero brings 8 columns instead of 4; no workspace, no extra pass, no allocation, no host
 *            synchronisation (after sextans_prepare_rm_bf16 the call can be captured into a hipGraph).  sextans_last_kernel =
 *            "spmm_csr_rowgroup_rowmajor_bf16" / "spmm_csr_rowgroup_rowmajor_bf16+long_rows" (bucketed long rows; split hub rows in
 *            SEXTANS_MODE_FAST).
 *   CONVERTED  everything else (LDS-panel and lane-per-row routes, exact chains, mixed plans, dense tiles, unaligned operands): B (and a
 *            bf16 C_in) are widened into fp32 workspaces of the engine, the fp32 row-major path runs, a bf16 C_out is rounded back.
 *            Correct for every matrix the fp32 entry accepts; sextans_last_kernel names the fp32 kernel that ran.  The workspaces
 *            (4 * K * N bytes, + 4 * M * N for a bf16 C) count in stat "device_bytes" and are dropped with the matrix.
 * Stats "bf16_native_calls" / "bf16_converted_calls": calls served either way since sextans_set_matrix_* (transposed calls included).
 * sextans_update_values* needs nothing more: the native kernels read the arrays a value refresh rewrites.
 * SEXTANS_ERR_INVALID: h / pointers NULL, N % 8, an ld < N, c_dtype unknown, an address that is not a multiple of its element size;
 * SEXTANS_ERR_STATE: no CSR matrix set.
 *   sextans_spmm_t_device_rm_bf16  the same for A^T (B is M x N, C is K x N), served by the companion engine of sextans_spmm_t_device_rm
 *       with this engine's options and value refreshes.
 *   sextans_prepare_rm_bf16  everything a later bf16 call for (N, c_dtype) would build or allocate, built now: the row-major plans of
 *       sextans_prepare(SEXTANS_LAYOUT_ROWMAJOR) -- transposed != 0: those of SEXTANS_LAYOUT_ROWMAJOR_T -- and, where a call with aligned
 *       operands converts, the fp32 workspaces.  (A call with UNALIGNED operands on a matrix whose aligned calls are native sizes its
 *       workspaces itself, at the call.) */
#define SEXTANS_DTYPE_F32 0
#define SEXTANS_DTYPE_BF16 1
int sextans_spmm_device_rm_bf16(sextans_handle_t h, int N, float alpha, const uint16_t *d_B, int64_t ldb, float beta, const void *d_C_in,
                                int64_t ldc_in, void *d_C_out, int64_t ldc, int c_dtype, void *stream);
int sextans_spmm_t_device_rm_bf16(sextans_handle_t h, int N, float alpha, const uint16_t *d_B, int64_t ldb, float beta, const void *d_C_in,
                                  int64_t ldc_in, void *d_C_out, int64_t ldc, int c_dtype, void *stream);
int sextans_prepare_rm_bf16(sextans_handle_t h, int N, int c_dtype, int transposed, void *stream);

/* ---- bf16 EDGE tensors for the edge-output ops and the edge-feature SpMM: the (nnz, N) tensors of a call -- E, Z and Gz of
 * sextans_edge_op*_device_rm, E and dE of sextans_spmm_edge*_device_rm -- in bf16 (16-bit patterns, uint16_t), read and written by the
 * kernels where they lie.  They are the binding traffic of both families (the node operands are 1 / degree of it); under autocast the
 * edge projection arrives in bf16 and the next layer wants bf16.  Closest thing in the reference: none.
 *
 * Storage changes, arithmetic does not.  The node tensors (xdst, xsrc, B, C, G, dxdst, dxsrc, dB) are fp32 as in the fp32 entry points,
 * so is every operation and every sum, in the same order (same tiles, slots and dealing).  ONE dtype for all edge tensors of a call:
 * there are no mixed forms.
 *     read    a bf16 value is widened exactly (16 zero bits appended)
 *     write   the fp32 result the fp32 entry point would have stored, rounded ONCE to nearest even: a NaN stays a quiet NaN, +-inf and
 *             -0 stay what they are, a finite fp32 value at or above the rounding boundary (0x7f7f8000) becomes inf
 * so for every op and pass
 *     a bf16 output (Z, dE) is round_bf16(the fp32 entry point's output on the widened inputs), bit for bit;
 *     an fp32 output (C, dxdst, dxsrc, dB) is the fp32 entry point's output on the widened inputs, bit for bit.
 * Arguments, ops, what a call reads and ignores, NULL rules, pass skipping ("no A^T without d_dxsrc" / "without d_dB"), degenerate
 * matrices and determinism are those of the fp32 twin (above).  No atomics, no workspace, no value refresh; after the first call on a
 * matrix -- in particular after sextans_prepare(h, N, SEXTANS_LAYOUT_ROWMAJOR_T, stream) -- a call allocates nothing, reads nothing back
 * and does not synchronise: it can be captured into a hipGraph.
 * Leading dimensions are counted in ELEMENTS of their tensor: >= N and multiples of 4 for the bf16 tensors too (a piece of 4 columns is
 * one 8-byte access), under the fp32 twin's rules for which of them count.  Every pointer 16-byte aligned.
 * sextans_last_kernel: "edge_op_bf16" / "edge_op_backward_bf16" / "spmm_edge_bf16" / "spmm_edge_backward_bf16", "+long_rows" appended
 * when the workgroup path ran.
 * Errors: the fp32 twin's, in its order (SEXTANS_ERR_INVALID for the arguments, then SEXTANS_ERR_STATE without a CSR matrix, then
 * SEXTANS_ERR_INVALID for nnz > INT32_MAX or a required pointer that is NULL with nnz > 0), all before any device is touched. */
int sextans_edge_op_device_rm_bf16(sextans_handle_t h, int op, int N, const float *d_xdst, int64_t ldxdst, const float *d_xsrc, int64_t ldxsrc,
                                   const uint16_t *d_E, int64_t lde, uint16_t *d_Z, int64_t ldz, void *stream);
int sextans_edge_op_backward_device_rm_bf16(sextans_handle_t h, int op, int N, const float *d_xdst, int64_t ldxdst, const float *d_xsrc,
                                            int64_t ldxsrc, const uint16_t *d_Gz, int64_t ldgz, float *d_dxdst, int64_t lddxdst,
                                            float *d_dxsrc, int64_t lddxsrc, void *stream);
int sextans_spmm_edge_device_rm_bf16(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const uint16_t *d_E, int64_t lde,
                                     float *d_C, int64_t ldc, void *stream);
int sextans_spmm_edge_backward_device_rm_bf16(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const uint16_t *d_E,
                                              int64_t lde, const float *d_G, int64_t ldg, float *d_dB, int64_t lddb, uint16_t *d_dE,
                                              int64_t ldde, void *stream);

/* The same for the two per-channel softmax families, the consumers of those tensors: S, D, dS and dD of
 * sextans_vector_attention*_device_rm, E and dE of sextans_spmm_edge_softagg*_device_rm in bf16, read and written where they lie.
 * The contract above, unchanged: ONE dtype for all edge tensors of a call; the node tensors (V, B, t, C, lse, G, dV, dB, dt and the dt
 * workspace), every operation, the online-softmax state and its merges are fp32, in the fp32 twin's order (same tiles, slots, entries in
 * flight and dealing).  A bf16 value is widened exactly -- a bf16 -inf score is still a mask: weight +0, dS = +0 --, a bf16 output is
 * the fp32 value the twin would have stored, rounded ONCE to nearest even (NaN stays a quiet NaN, +-inf and -0 stay, a value at or
 * above 0x7f7f8000 becomes inf).  So for every mode / op and pass
 *     a bf16 output (dS, dD, dE) is round_bf16(the fp32 entry point's output on the widened inputs), bit for bit;
 *     an fp32 output (C, lse, dV, dB, dt) is the fp32 entry point's output on the widened inputs, bit for bit.
 * Arguments, modes / ops, what a call reads and ignores, NULL rules, pass skipping, degenerate matrices and determinism are the fp32
 * twin's.  No atomics, no value refresh, no workspace beyond the twin's: sextans_spmm_edge_softagg_workspace_floats serves both dtypes.
 * Capturable into a hipGraph after sextans_prepare(h, N, SEXTANS_LAYOUT_ROWMAJOR_T, stream), as the twins are.
 * Leading dimensions are counted in ELEMENTS of their tensor: >= N and multiples of 4 for the bf16 tensors too, under the twin's rules
 * for which of them count.  Every pointer 16-byte aligned.
 * sextans_last_kernel: "vector_attention_bf16" / "vector_attention_backward_bf16" / "spmm_edge_softagg_bf16" /
 * "spmm_edge_softagg_backward_bf16", "+long_rows" appended when the workgroup path ran.
 * Errors: the fp32 twin's, in its order, all before any device is touched. */
int sextans_vector_attention_device_rm_bf16(sextans_handle_t h, int msg, int N, const uint16_t *d_S, int64_t lds, const float *d_V, int64_t ldv,
                                            const uint16_t *d_D, int64_t ldd, float *d_C, int64_t ldc, float *d_lse, int64_t ldlse,
                                            void *stream);
int sextans_vector_attention_backward_device_rm_bf16(sextans_handle_t h, int msg, int N, const uint16_t *d_S, int64_t lds, const float *d_V,
                                                     int64_t ldv, const uint16_t *d_D, int64_t ldd, const float *d_C, int64_t ldc,
                                                     const float *d_lse, int64_t ldlse, const float *d_G, int64_t ldg, uint16_t *d_dS,
                                                     int64_t ldds, float *d_dV, int64_t lddv, uint16_t *d_dD, int64_t lddd, void *stream);
int sextans_spmm_edge_softagg_device_rm_bf16(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const uint16_t *d_E, int64_t lde,
                                             const float *d_t, float *d_C, int64_t ldc, float *d_lse, int64_t ldlse, void *stream);
int sextans_spmm_edge_softagg_backward_device_rm_bf16(sextans_handle_t h, int op, int N, const float *d_B, int64_t ldb, const uint16_t *d_E,
                                                      int64_t lde, const float *d_t, const float *d_C, int64_t ldc, const float *d_lse,
                                                      int64_t ldlse, const float *d_G, int64_t ldg, float *d_dB, int64_t lddb, uint16_t *d_dE,
                                                      int64_t ldde, float *d_dt, float *d_work, void *stream);

/* The same for the gated aggregation (GatedGCN / ResGatedGraphConv), in which the (nnz, N) tensors weigh most: E, z, Gz and dE of
 * sextans_spmm_gated*_device_rm in bf16, read and written where they lie.  The contract above, unchanged: ONE dtype for all edge
 * tensors of a call; everything of node size (xdst, xsrc, V, C, den, G, the gn workspace, dxdst, dxsrc, dV), every operation, every sum
 * and every merge are fp32, in the fp32 twin's order (same tiles, slots, entries in flight and dealing).  A bf16 value is widened
 * exactly, a bf16 output is the fp32 value the twin would have stored, rounded ONCE to nearest even (NaN stays a quiet NaN, +-inf and
 * -0 stay, a value at or above 0x7f7f8000 becomes inf).  The rounded value never feeds back: the gate is computed from the unrounded
 * fp32 z_e in all three passes, and dxdst and dxsrc sum the unrounded fp32 dz_e.  So for either mode and every pass
 *     a bf16 output (z, dE) is round_bf16(the fp32 entry point's output on the widened inputs), bit for bit;
 *     an fp32 output (C, den, dxdst, dxsrc, dV) is the fp32 entry point's output on the widened inputs, bit for bit.
 * The structs have the layouts of sextans_gated_in / sextans_gated_grad.  Arguments, modes, what a call reads and ignores, NULL rules
 * (d_e == NULL with a d_z: z without E, rounded; d_de without d_e: the gradient of z), pass skipping, degenerate matrices and
 * determinism are the fp32 twin's.  No atomics, no value refresh, no workspace beyond the twin's: sextans_spmm_gated_workspace_floats
 * serves both dtypes.  Capturable into a hipGraph after sextans_prepare(h, N, SEXTANS_LAYOUT_ROWMAJOR_T, stream), as the twins are.
 * Leading dimensions are counted in ELEMENTS of their tensor: >= N and multiples of 4 for the bf16 tensors too, under the twin's rules
 * for which of them count.  Every pointer 16-byte aligned.
 * sextans_last_kernel: "spmm_gated_bf16" / "spmm_gated_backward_bf16", "+long_rows" appended when the workgroup path ran.
 * Errors: the fp32 twin's, in its order, all before any device is touched. */
typedef struct { const float *d_xdst, *d_xsrc, *d_v; const uint16_t *d_e; int64_t ld_xdst, ld_xsrc, ld_v, ld_e; } sextans_gated_in_bf16;
typedef struct { float *d_dxdst, *d_dxsrc, *d_dv; uint16_t *d_de; int64_t ld_dxdst, ld_dxsrc, ld_dv, ld_de; } sextans_gated_grad_bf16;
int sextans_spmm_gated_device_rm_bf16(sextans_handle_t h, int mode, float eps, int N, const sextans_gated_in_bf16 *in,
                                      float *d_C, int64_t ldc, float *d_den, int64_t ldden, uint16_t *d_z, int64_t ldz, void *stream);
int sextans_spmm_gated_backward_device_rm_bf16(sextans_handle_t h, int mode, float eps, int N, const sextans_gated_in_bf16 *in,
                                               const float *d_C, int64_t ldc, const float *d_den, int64_t ldden,
                                               const float *d_G, int64_t ldg, const uint16_t *d_Gz, int64_t ldgz,
                                               const sextans_gated_grad_bf16 *out, float *d_work, void *stream);

/* Row-range form: computes rows [row_begin, row_end) only.  d_C_in / d_C_out address row_begin as
 * their row 0 (ldc_in, ldc_out >= row_end - row_begin).  Used to pipeline a rank's slab in chunks so the
 * all-gather of chunk i overlaps the SpMM of chunk i+1.  flags: SEXTANS_ROWS_REUSE_B_PANELS = the B
 * panels repacked by the previous call on this handle are still valid (same B, same N): skip the repack.
 * A range that starts and ends on sextans_align_row boundaries (or at 0 / M) keeps the whole-matrix kernel;
 * any other range uses the row-group gather kernel. */
#define SEXTANS_ROWS_REUSE_B_PANELS 1
int sextans_spmm_device_rows(sextans_handle_t h, int N, float alpha, const float *d_B, int64_t ldb,
                             float beta, const float *d_C_in, int64_t ldc_in, float *d_C_out,
                             int64_t ldc_out, int row_begin, int row_end, int flags, void *stream);

/* Largest row <= `row` at which a row-range call of an N-column SpMM on this matrix can be cut without losing
 * the kernel the dispatcher would use for the whole matrix (a wavefront boundary of the window kernel, a row
 * block boundary of the LDS-panel kernel; any row for the gather kernel).  row == M is returned unchanged.
 * Builds the packed forms of A if they do not exist yet. */
int sextans_align_row(sextans_handle_t h, int N, int row, int *aligned);

/* Drop-in for the kernel-invoke call itself: the argument list of
 *   tapa::invoke(Sextans, bitstream, edge_list_ptr, edge_list_ch[8], mat_B_ch[NUM_CH_B], mat_C_ch_in[8],
 *                mat_C_ch[8], NUM_ITE, NUM_A_LEN, M, K, P_N, alpha_u, beta_u)
 * (sextans-host.cpp:237-251, prototype sextans.h:20-26) on the host buffers the reference host prepared.
 * P_N = (rp_time << 16) | N, alpha_u / beta_u = fp32 bit patterns.  The stream is decoded and uploaded
 * (edge_list_ptr == NULL: keep the matrix set by the previous sextans_set_matrix_edges / sextans_invoke on
 * this handle, which must have the same M and K); B and C_in channels are uploaded and converted on the
 * device; C_out channels receive colsize * N/8 floats each, padded rows included (alpha*0 + beta*0, as the
 * accelerator writes them).  *elapsed_ns = device time of the layout conversions + all rp_time repeats.
 * Results are bit-identical to cpu_spmm_CSR on the decoded matrix. */
int sextans_set_matrix_edges(sextans_handle_t h, const int32_t *edge_list_ptr, const uint64_t *const *edge_list_ch,
                             int NUM_ITE, int NUM_A_LEN, int M, int K);
int sextans_invoke(sextans_handle_t h, const int32_t *edge_list_ptr, const uint64_t *const *edge_list_ch,
                   const float *const *mat_B_ch, int num_ch_b, const float *const *mat_C_ch_in,
                   float *const *mat_C_ch, int NUM_ITE, int NUM_A_LEN, int M, int K, int P_N, int alpha_u,
                   int beta_u, double *elapsed_ns);

/* ---- Multi-GPU form behind the C ABI (north_star: A row-range partitioned across the GPUs of one node, B
 * replicated, RCCL all-gather of C panels over xGMI).  The reference is single-device; its only
 * sharding is rows -> PEs with B broadcast (sparse_helper.h:370, sextans.cpp:916-927), the same independence of
 * output rows used here.  One process (or thread) per GPU; RCCL is bound at run time (librccl.so.1, or the
 * library named by SEXTANS_RCCL_PATH), so single-GPU callers never need it.
 *
 *   sextans_dist_unique_id   rank 0 creates the 128-byte RCCL id and hands it to the other ranks by its own
 *                            means (MPI_Bcast, a file, a socket);
 *   sextans_dist_comm_init   every rank: communicator of `world` ranks on HIP device `device`;
 *   sextans_dist_spmm        the engine holds THIS rank's rows [row_ranges[2*rank], row_ranges[2*rank+1]) of the
 *                            M_total x K matrix (ranges tile [0, M_total) in rank order, unequal lengths allowed:
 *                            nnz-balanced splits); d_B is the full K x N matrix, d_C_in / d_C_out the full
 *                            column-major M_total x N matrices on this rank's device.  The rank's slab is
 *                            computed in `nchunks` row chunks (cut at sextans_align_row boundaries, exchanged between
 *                            the ranks once per partition) into a staging buffer; the all-gather of chunk i
 *                            (ncclAllGather on the engine's communication stream) overlaps the SpMM of chunk
 *                            i+1; a final pass writes every rank's rows into d_C_out.  Enqueued on `stream`,
 *                            returns without synchronising (host syncs only the first time a partition is used:
 *                            cut exchange and row tables).  d_C_out holds C = alpha*A*B + beta*C_in for ALL rows on
 *                            every rank.
 *                            CLUSTERED-ORDER CHUNKS (round 5): a rank whose slab runs on a graph-clustered plan ("row_cluster":
 *                            a renumbered mesh) keeps the reordered form with nchunks > 1 -- a chunk is then a range of the plan's
 *                            row blocks, its packed slab holds the rows in clustered order, and every rank scatters the received
 *                            slabs through the senders' position -> row tables (exchanged once per partition) into a row-major
 *                            staging copy of C that one streaming pass turns into column-major d_C_out.  Used when every rank of
 *                            the partition can (one flag per rank is exchanged); N % 16 == 0.
 *                            comm == NULL with world == 1: the same pipeline without collectives (single-GPU callers without RCCL). */
/* Contiguous row ranges with (nearly) equal non-zero counts for `world` ranks: ranges[2g], ranges[2g+1] = rows of rank g
 * (split points by binary search in row_ptr; host function, no device needed). */
int sextans_partition_rows_by_nnz(int M, const int *row_ptr, int world, int *ranges);
/* Which library the collectives come from (round 6).  By default the first of $SEXTANS_RCCL_PATH, librccl.so.1, /opt/rocm/lib/librccl.so.1,
 * librccl.so that dlopen finds, bound at the first use.  sextans_dist_bind_library(path) binds `path` instead (NULL or "": back to the
 * default search) -- a site's own RCCL build, or the loopback communicator of this repository's tests (tests/fake_rccl.cpp: ranks as
 * threads of one process on one device, so that world > 1 runs on a single-GPU box).  The library must export ncclGetUniqueId,
 * ncclCommInitRank, ncclCommDestroy, ncclAllGather (and ncclBroadcast, ncclGroupStart, ncclGroupEnd for row-major slabs of unequal
 * length).  SEXTANS_ERR_STATE while communicators created through sextans_dist_comm_init are alive. */
int sextans_dist_bind_library(const char *path);
/* Everything a sextans_dist_spmm* call would otherwise do INSIDE ITS FIRST INVOCATION for a partition -- exchange of the ranks' non-zero
 * counts (long-row thresholds follow the whole matrix), "row_offset", the plan build of this rank's slab (0.3-0.7 s for 3e8 non-zeros),
 * the cut-list / clustered-order flag / position -> row table exchanges of the chunk pipeline, workspaces, streams and events -- as ONE
 * collective call outside any timed region.  `form` selects the entry point it prepares for:
 *   SEXTANS_DIST_CSR_COLMAJOR  sextans_dist_spmm      (nchunks as in that call)
 *   SEXTANS_DIST_CSR_ROWMAJOR  sextans_dist_spmm_rm   (nchunks ignored; ldc of the later call assumed == N unless nchunks < 0: packed copy)
 *   SEXTANS_DIST_BELL          sextans_dist_spmm_bell (nchunks ignored)
 * Every rank of the communicator must call it (it is a collective).  It ends with an exchange of the ranks' status: it returns
 * SEXTANS_OK on ALL ranks or an error on ALL ranks -- a rank whose own work failed gets its own code, the others SEXTANS_ERR_PEER --
 * and no rank is left waiting in a collective for a rank that gave up.  After it, the dist call for the same (ranges, N, nchunks)
 * performs no host synchronisation and no control collective (stat "dist_setup_exchanges" stays where it was).  Optional: the dist
 * calls still prepare lazily when it was not called.  comm == NULL with world == 1: the local part alone. */
#define SEXTANS_DIST_CSR_COLMAJOR 0
#define SEXTANS_DIST_CSR_ROWMAJOR 1
#define SEXTANS_DIST_BELL 2
int sextans_dist_prepare(sextans_handle_t h, void *comm, int world, int rank, const int *row_ranges, int N, int nchunks, int form, void *stream);
int sextans_dist_unique_id(char id[128]);
int sextans_dist_comm_init(void **comm, int device, int world, int rank, const char id[128]);
int sextans_dist_comm_destroy(void *comm);
int sextans_dist_spmm(sextans_handle_t h, void *comm, int world, int rank, const int *row_ranges, int N, float alpha,
                      const float *d_B, int64_t ldb, float beta, const float *d_C_in, int64_t ldc_in, float *d_C_out,
                      int64_t ldc, int nchunks, void *stream);
/* The same for ROW-major operands (round 5; d_B K x N with ldb >= N, d_C_in / d_C_out M_total x N with ldc_in / ldc >= N, all of it on
 * every rank): the rank's rows are computed by sextans_spmm_device_rm straight into their place in d_C_out -- rows [r0, r1) of a
 * row-major matrix with ldc == N are ONE contiguous run -- and exchanged by an in-place all-gather on `stream` (ncclAllGather for
 * ranges of equal length, a group of ncclBroadcast otherwise): no repack of the replicated B on every rank, no staging buffer, no
 * unpack pass, and every plan kind (natural, bricks, graph-clustered) keeps its whole-slab kernel.  ldc > N: through a packed copy.
 * C_in is read in this rank's rows only.  comm == NULL with world == 1: the SpMM alone. */
int sextans_dist_spmm_rm(sextans_handle_t h, void *comm, int world, int rank, const int *row_ranges, int N, float alpha, const float *d_B,
                         int64_t ldb, float beta, const float *d_C_in, int64_t ldc_in, float *d_C_out, int64_t ldc, void *stream);

/* One-shot convenience with exactly cpu_spmm_CSR's argument list (sparse_helper.h:262-272):
 * create + upload + run + download + destroy on device 0. */
int sextans_spmm_csr(int M, int N, int K, int NNZ, float ALPHA, const int *CSRRowPtr,
                     const int *CSRColIndex, const float *CSRVal, const float *mat_B, float BETA,
                     float *mat_C);

/* ---- Blocked-ELL bf16 path (BASELINE config 5; no counterpart in the reference, whose PEs are scalar
 * fp32 MACs): A is M x K in dense 32x32 bf16 blocks, `ell_width` block slots per block row;
 * block_col[br*ell_width + s] is the block column of slot s (or -1 = empty slot), block_val holds the
 * slots' 32x32 bf16 values row-major (1024 values per slot).  B is bf16 COLUMN MAJOR K x N (ldb % 8 == 0),
 * C fp32 column major, C = alpha*A*B + beta*C with fp32 accumulation on v_mfma_f32_32x32x16_bf16.
 * M, K, N must be multiples of 32.  bf16 values are passed as their 16-bit patterns (uint16_t).
 * beta = 0 does NOT mask C_in: every kernel variant evaluates (alpha * acc) + (beta * C_in) as written, so a NaN or an infinity in
 * C_in arrives in C_out as NaN at beta = 0 too (0 * NaN = 0 * inf = NaN) -- cpu_spmm_CSR's contract (sparse_helper.h:287), the
 * same on spmm_bell_mfma<1|2|4>, _n256 and _shared and on the dense-tile route; pass a finite C_in (it may alias C_out).
 * Leading dimensions: only rows [0, K) of each column of B are read and only rows [0, M) of each column of C_out are written --
 * whatever lies between K and ldb, or M and ldc, is neither read nor touched.  (tests/test_bell_exact_gpu.py pins both.) */
int sextans_set_matrix_bell(sextans_handle_t h, int M, int K, int ell_width, const int *block_col,
                            const uint16_t *block_val);
int sextans_set_matrix_bell_device(sextans_handle_t h, int M, int K, int ell_width,
                                   const int *d_block_col, const uint16_t *d_block_val);
int sextans_spmm_bell_device(sextans_handle_t h, int N, float alpha, const uint16_t *d_B, int64_t ldb,
                             float beta, const float *d_C_in, float *d_C_out, int64_t ldc, void *stream);
/* The same with separate leading dimensions for C_in and C_out (a rank of sextans_dist_spmm_bell reads its rows inside the whole C_in
 * and writes a packed slab). */
int sextans_spmm_bell_device2(sextans_handle_t h, int N, float alpha, const uint16_t *d_B, int64_t ldb, float beta, const float *d_C_in,
                              int64_t ldc_in, float *d_C_out, int64_t ldc, void *stream);
/* Blocked-ELL over the GPUs of one node (block-row ranges): the engine holds the block rows of
 * [row_ranges[2*rank], row_ranges[2*rank+1]) -- multiples of 32, tiling [0, M_total) in rank order -- d_B is the whole bf16 K x N matrix,
 * d_C_in / d_C_out the whole column-major fp32 M_total x N matrices on this rank's device.  The rank's slab is written packed into a
 * staging buffer, one ncclAllGather on `stream` moves all slabs, one pass writes d_C_out: complete on every rank, stream-ordered,
 * bit-identical to sextans_spmm_bell_device on the whole matrix.  comm == NULL with world == 1: no collective. */
int sextans_dist_spmm_bell(sextans_handle_t h, void *comm, int world, int rank, const int *row_ranges, int N, float alpha, const uint16_t *d_B,
                           int64_t ldb, float beta, const float *d_C_in, int64_t ldc_in, float *d_C_out, int64_t ldc, void *stream);

/* Per-kernel device timing collected while option "profile" = 1: mean duration in ns of the
 * dominant SpMM kernel launches since the last reset, and how many were timed. */
int sextans_profile_read(sextans_handle_t h, double *mean_kernel_ns, int64_t *launches,
                         double *mean_repack_ns);
/* Mean duration of what a call launches BEHIND its SpMM kernel (the reordered form's C staging -> C pass); 0 launches otherwise. */
int sextans_profile_read_post(sextans_handle_t h, double *mean_post_ns, int64_t *launches);
int sextans_profile_reset(sextans_handle_t h);

/* Debug aid (option "phase_timing" = 1): wave cycles of the panel kernel's phases summed over a 1/128
 * sample of workgroups: {meta+extents+first entries, dictionary->B rows->LDS, row streaming, C tile
 * + epilogue, sampled waves, 0, 0, 0} since the option was set. */
int sextans_phase_timing_read(sextans_handle_t h, int64_t out[8]);

/* Name of the kernel the dispatcher last used (static string), for logs and rocprof matching. */
const char *sextans_last_kernel(sextans_handle_t h);

/* ------------------------------------------------------------------ synthetic inputs (bench) */

/* Deterministic counter-based synthetic CSR (BASELINE config 4): row lengths Poisson(mean_nnz)
 * from an integer inverse-CDF table, columns uniform without replacement and sorted (bandwidth 0:
 * over [0,K); bandwidth bw > 0: over the band [row-bw, row+bw], a FEM/SuiteSparse-like matrix with
 * locality), values U(-1,1).  Host and device generators produce identical bits for the same (seed,row).
 * Host form generates rows [r0,r1) only (row_ptr has r1-r0+1 entries starting at 0). */
int sextans_gen_csr_host(int M, int K, double mean_nnz, int bandwidth, uint64_t seed, int r0, int r1,
                         int **row_ptr, int **col_idx, float **val, int64_t *nnz);
/* Device form: allocates device arrays on `device` (free with sextans_device_free). */
int sextans_gen_csr_device(int device, int M, int K, double mean_nnz, int bandwidth, uint64_t seed, int r0,
                           int r1, int **d_row_ptr, int **d_col_idx, float **d_val, int64_t *nnz);
/* 3-D finite-element-like matrix: 27-point node stencil on an nx*ny*nz grid with `dof` unknowns per
 * node (dense dof x dof coupling blocks), M = K = nx*ny*nz*dof, values U(-1,1).  Stand-in for
 * SuiteSparse FEM inputs that cannot be downloaded here (Boeing/pcrystk02 = 13965 rows, 3 dof,
 * ~69 nnz/row is reproduced by 19 x 15 x 16 x 3 + trimming). */
int sextans_gen_fem3d_host(int nx, int ny, int nz, int dof, uint64_t seed, int r0, int r1, int **row_ptr,
                           int **col_idx, float **val, int64_t *nnz);
int sextans_gen_fem3d_device(int device, int nx, int ny, int nz, int dof, uint64_t seed, int r0, int r1,
                             int **d_row_ptr, int **d_col_idx, float **d_val, int64_t *nnz);
/* Power-law matrix (the sweep harness's load-balancing case): row lengths with
 * P(len >= x) = (xmin / x)^(tail_x100 / 100) on [xmin, min(max_len, K)] -- a few hub rows hundreds of thousands
 * of entries long next to a mass of short rows -- columns one uniform draw per equal stratum of [0, K) (distinct,
 * ascending), values U(-1,1).  Same bits on host and device. */
/* 2-D stencil (points = 5 or 9) on an nx x ny grid with dof unknowns per node; KKT / arrow block structure
 * [[H, A^T, U], [A, 0, U], [V, V, D]] with n variables (pentadiagonal H), n/2 constraints of 3 variables each and `arrow`
 * border rows/columns (border rows hold every 16th column: a few very long rows).  Same bits on host and device. */
int sextans_gen_stencil2d_host(int nx, int ny, int points, int dof, uint64_t seed, int r0, int r1, int **row_ptr, int **col_idx,
                               float **val, int64_t *nnz);
int sextans_gen_stencil2d_device(int device, int nx, int ny, int points, int dof, uint64_t seed, int r0, int r1, int **d_row_ptr,
                                 int **d_col_idx, float **d_val, int64_t *nnz);
/* P A P^T of a device-resident CSR matrix (measurement infrastructure for meshes in arbitrary node orders): row / column i becomes
 * row / column new_of_old[i] (host array, a permutation of 0 .. M-1), columns ascending per row, values travel with their entries.
 * New device arrays (sextans_device_free).  Rows of up to 4096 entries. */
int sextans_csr_permute_symmetric_device(int device, int M, int64_t nnz, const int *d_row_ptr, const int *d_col_idx, const float *d_val,
                                         const int *new_of_old, int **o_row_ptr, int **o_col_idx, float **o_val);
/* Rows [r0, r1) of a device-resident CSR matrix as a matrix of their own (what a rank of the row-partitioned SpMM holds; measurement
 * infrastructure): a new row_ptr of r1 - r0 + 1 entries starting at 0 (sextans_device_free), *first_entry = where the slab's
 * col_idx / val begin inside the original arrays (use d_col_idx + *first_entry, d_val + *first_entry), *nnz = its non-zeros. */
int sextans_csr_slice_rows_device(int device, int r0, int r1, const int *d_row_ptr, int **o_row_ptr, int64_t *first_entry, int64_t *nnz);
/* HOLDOUT class (round 5): kron(T_n, P) -- n copies of a caller-given pm x pk sparsity pattern P (the tests and the bench pass the
 * pattern of a real SuiteSparse matrix, nasa4704) on the block diagonal, each coupled to its neighbours through the same pattern
 * (T_n tridiagonal): M = n * pm rows, row i * pm + p holds the columns j * pk + P[p][*] for j = i - 1, i, i + 1; values U(-1,1) from the
 * counter RNG (halved in the off-diagonal blocks).  `variant` bits: 1 = rectangular (every third column dropped, the rest renumbered:
 * K = 2/3 of n * pk), 2 = unsymmetric pattern (30 % of the strictly lower entries dropped).  *K_out = columns of the result.  The
 * pattern arrays are HOST pointers in both forms.  Same bits on host and device; any row range [r0, r1). */
int sextans_gen_kron_host(int n, int pm, int pk, const int *p_row_ptr, const int *p_col_idx, int variant, uint64_t seed, int r0, int r1,
                          int **row_ptr, int **col_idx, float **val, int64_t *nnz, int *K_out);
int sextans_gen_kron_device(int device, int n, int pm, int pk, const int *p_row_ptr, const int *p_col_idx, int variant, uint64_t seed,
                            int r0, int r1, int **d_row_ptr, int **d_col_idx, float **d_val, int64_t *nnz, int *K_out);
int sextans_gen_kkt_host(int n, int arrow, uint64_t seed, int r0, int r1, int **row_ptr, int **col_idx, float **val, int64_t *nnz);
int sextans_gen_kkt_device(int device, int n, int arrow, uint64_t seed, int r0, int r1, int **d_row_ptr, int **d_col_idx,
                           float **d_val, int64_t *nnz);
int sextans_gen_powerlaw_host(int M, int K, int xmin, int tail_x100, int max_len, uint64_t seed, int r0, int r1,
                              int **row_ptr, int **col_idx, float **val, int64_t *nnz);
int sextans_gen_powerlaw_device(int device, int M, int K, int xmin, int tail_x100, int max_len, uint64_t seed, int r0,
                                int r1, int **d_row_ptr, int **d_col_idx, float **d_val, int64_t *nnz);
/* Blocked-ELL synthetic input (BASELINE config 5): every block row gets `ell_width` distinct sorted
 * block columns, values bf16(U(-1,1)).  Device form allocates (free with sextans_device_free). */
int sextans_gen_bell_host(int M, int K, int ell_width, uint64_t seed, int **block_col, uint16_t **block_val);
int sextans_gen_bell_device(int device, int M, int K, int ell_width, uint64_t seed, int **d_block_col,
                            uint16_t **d_block_val);
/* Block-banded blocked-ELL (ell_width = 2 * half_width + 1 consecutive block columns around the diagonal block, window
 * shifted inwards at the edges): block rows share block columns, the case spmm_bell_mfma_shared is built for. */
int sextans_gen_bell_banded_host(int M, int K, int half_width, uint64_t seed, int **block_col, uint16_t **block_val);
int sextans_gen_bell_banded_device(int device, int M, int K, int half_width, uint64_t seed, int **d_block_col,
                                   uint16_t **d_block_val);
/* bf16(U(-1,1)) fill (same bits on host and device). */
int sextans_gen_uniform_bf16_host(uint16_t *dst, int64_t n, uint64_t seed);
int sextans_gen_uniform_bf16_device(int device, uint16_t *d_dst, int64_t n, uint64_t seed, void *stream);
/* U(-1,1) fp32 fill, element i of stream `seed` (same bits on host and device). */
int sextans_gen_uniform_host(float *dst, int64_t n, uint64_t seed);
int sextans_gen_uniform_device(int device, float *d_dst, int64_t n, uint64_t seed, void *stream);
int sextans_device_free(int device, void *d_ptr);
/* Device memory helpers for callers of the device generators that have no HIP binding of their own (Python tools, the bench): they go
 * through the ONE HIP runtime this library is linked against -- a second dlopen("libamdhip64.so") by another name can map a second
 * runtime whose calls fail on this one's pointers.  Synchronous with respect to the host; kind = SEXTANS_COPY_*. */
#define SEXTANS_COPY_HOST_TO_DEVICE 1
#define SEXTANS_COPY_DEVICE_TO_HOST 2
#define SEXTANS_COPY_DEVICE_TO_DEVICE 3
int sextans_device_alloc(int device, size_t bytes, void **d_ptr);
int sextans_device_copy(int device, void *dst, const void *src, size_t bytes, int kind);

#ifdef __cplusplus
}
#endif
#endif /* SEXTANS_AMD_H */
