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
// There is NO CPU fallback anywhere in the engine: no device => SEXTANS_ERR_NO_DEVICE.
// This unit: handles, the option table, matrices, stats, plan / row-order export, profiling reads, sextans_device_*.  The SpMM entry
// points and the launch layer they share are units of their own (file map: engine_state.h).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "engine_launch.h"
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

// Every option, declared once: key, slot (default and meaning: engine_state.h), what a CHANGE of it invalidates, whether it is a
// measurement switch, and the values it takes -- a range [lo, hi], or `only`: bit v set for every allowed value v.
enum Drops { kNothing, kWindowStream, kClusterPlan, kPackedPlans, kColwiseVerdict };   // kClusterPlan: and cluster_rm_tried
constexpr int64_t kMin = INT64_MIN, kMax = INT64_MAX;
using E = sextans_engine;
static const struct Option {
    const char *key; int64_t E::*slot; Drops drops = kNothing; bool measurement = false; int64_t lo = kMin, hi = kMax; uint64_t only = 0;
} kOptions[] = {
    // any value, nothing dropped
    {"kernel", &E::opt_kernel}, {"stage_a", &E::opt_stage}, {"xcd_remap", &E::opt_xcd}, {"exact", &E::opt_exact}, {"profile", &E::opt_profile},
    {"split_rows", &E::opt_split_rows}, {"bucket_rows", &E::opt_bucket_rows}, {"global_nnz", &E::opt_global_nnz}, {"exact_chain", &E::opt_exact_chain},
    {"fuse_b", &E::opt_fuse_b}, {"small_v2", &E::opt_small_v2}, {"colwise_tiles_adjacent", &E::opt_colwise_tiles_adjacent}, {"window_auto", &E::opt_win_auto},
    {"bell_wide", &E::opt_bell_wide}, {"bell_generation", &E::opt_bell_gen}, {"bell_shared", &E::opt_bell_shared}, {"mfma_dense_tiles", &E::opt_mfma_dense},
    {"dense_tile_fill_x100", &E::opt_dense_fill_x100},
    // a range or a set of values
    {"lanes_per_row", &E::opt_lpr, kNothing, false, kMin, kMax, 1 | 1 << 2 | 1 << 4 | 1 << 8},
    {"cols_per_lane", &E::opt_cols_per_lane, kNothing, false, kMin, kMax, 1 | 1 << 4 | 1 << 8},
    {"window_unroll", &E::opt_win_unroll, kNothing, false, kMin, kMax, 1 << 4 | 1 << 8},
    {"tiles_per_wg", &E::opt_tiles_per_wg, kNothing, false, 0, 1024}, {"panel_v2", &E::opt_panel_v2, kNothing, false, -1, 1},
    // measurement switches
    {"phase_timing", &E::opt_phase_timing, kNothing, true}, {"reordered_xcd", &E::opt_reordered_xcd, kNothing, true}, {"bell_debug", &E::opt_bell_debug, kNothing, true},
    {"dist_broadcast_runs", &E::opt_dist_broadcast_runs, kNothing, true}, {"rowblock_tiles", &E::opt_rb_tiles, kNothing, true},
    {"cluster_shape", &E::opt_cluster_shape, kClusterPlan, true},   // (its factors: checked in sextans_set_option)
    {"cluster_group", &E::opt_cluster_group, kClusterPlan, true, 1, 64},
    // the clustered-order plan is (re)considered under the new setting
    {"panel_min_reuse_x100", &E::opt_min_reuse_x100, kClusterPlan}, {"panel_min_reuse_wide_x100", &E::opt_min_reuse_wide_x100, kClusterPlan},
    {"row_cluster", &E::opt_row_cluster, kClusterPlan, false, -1, 2}, {"row_similarity", &E::opt_row_similarity, kClusterPlan, false, -1, 1},
    {"cluster_top", &E::opt_cluster_top, kClusterPlan}, {"small_panel", &E::opt_small_panel, kClusterPlan}, {"row_sets", &E::opt_row_sets, kClusterPlan},
    {"row_offset", &E::opt_row_offset, kClusterPlan}, {"relabel_columns", &E::opt_relabel_columns, kClusterPlan}, {"run_cluster", &E::opt_run_cluster, kClusterPlan},
    {"refine_sweeps", &E::opt_refine_sweeps, kClusterPlan}, {"refine_rows", &E::opt_refine_rows, kClusterPlan},
    // the stream is built for one (rows per wavefront, window) pair
    {"window_rows", &E::opt_win_rows, kWindowStream, false, 1, sx::kWinMaxRowsPerWave}, {"window_cols", &E::opt_win_cols, kWindowStream, false, 1, 0x7fffffff},
    // (every packed form is rebuilt; "split_mixed" moves the share of blocks with reuse from which a mixed plan is built at all, and a
    // cached "not built" verdict or a plan built under the other threshold must not survive the toggle)
    {"share_index", &E::opt_share_index, kPackedPlans}, {"split_mixed", &E::opt_split_mixed, kPackedPlans},
    {"colwise_max_len", &E::opt_colwise_max_len, kColwiseVerdict},
};

static const Option *find_option(const char *key) {
    for (const Option &o : kOptions)
        if (!strcmp(key, o.key)) return &o;
    return nullptr;
}

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
    preload_device_code();   // (the runtime loads it lazily at the first launch, ~1 ms, which would otherwise land inside the first timed SpMM)
    *out = h;
    return SEXTANS_OK;
}

int sextans_destroy(sextans_handle_t h) {
    if (!h) return SEXTANS_ERR_INVALID;
    (void)hipSetDevice(h->device);
    free_matrix(h);
    free_bell(h);
    sextans_profile_reset(h);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    if (h->aux_stream) (void)hipStreamDestroy(h->aux_stream);
    for (hipEvent_t e : h->dist_events) (void)hipEventDestroy(e);
    if (h->comm_stream) (void)hipStreamDestroy(h->comm_stream);
    if (h->host_stream) (void)hipStreamDestroy(h->host_stream);
    delete h;   // (the workspaces go with it: on h->device, set above)
    return SEXTANS_OK;
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
    const Option *o = find_option(key);
    if (!o) return SEXTANS_ERR_INVALID;
    int64_t *slot = &(h->*o->slot);
    // Measurement switches -- ablation bits that corrupt C on purpose ("bell_debug"), brick shapes and groupings of the clustered
    // row order, per-phase cycle counters -- are not part of the drop-in surface: they exist only for processes started with
    // SEXTANS_DEBUG_OPTIONS=1 (tools/), and a value other than the default is refused otherwise.
    if (o->measurement) {
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
    if (value < o->lo || value > o->hi || (o->only && (value < 0 || value > 63 || !(o->only >> value & 1)))) return SEXTANS_ERR_INVALID;
    if (*slot != value) {
        if (o->drops != kNothing && o->drops != kColwiseVerdict) (void)hipSetDevice(h->device);   // (the forms below are freed on the engine's device)
        switch (o->drops) {
            case kWindowStream: free_window(h); break;
            case kClusterPlan: free_cluster_plan(h); h->cluster_rm_tried = false; break;
            case kPackedPlans: free_plan(h); break;
            case kColwiseVerdict: h->cluster.colwise_state = 0; break;
            case kNothing: break;
        }
        h->dist_cut_key.clear();   // chunk cuts are aligned to the packed forms the options select (all ranks of a partition must change
                                   // options together: the cut exchange is a collective)
    }
    *slot = value;
    if (slot == &h->opt_phase_timing) {
        (void)hipSetDevice(h->device);
        if (value && h->d_dbg.reserve(8) != hipSuccess) return SEXTANS_ERR_HIP;
        if (h->d_dbg) (void)hipMemset(h->d_dbg, 0, 64);
        if (!value) h->d_dbg.reset();
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
    const Option *o = find_option(key);
    if (!o) return SEXTANS_ERR_INVALID;
    *value = h->*o->slot;
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
    DevBuf<int> rp, ci;
    DevBuf<float> v;
    SX_HIP(rp.alloc((size_t)M + 1));
    SX_HIP(ci.alloc((size_t)nnz));
    SX_HIP(v.alloc((size_t)nnz));
    SX_HIP(hipMemcpy(rp, row_ptr, sizeof(int) * ((size_t)M + 1), hipMemcpyHostToDevice));
    if (nnz) {
        SX_HIP(hipMemcpy(ci, col_idx, sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice));
        SX_HIP(hipMemcpy(v, val, sizeof(float) * (size_t)nnz, hipMemcpyHostToDevice));
    }
    h->mat.d_rp_own = std::move(rp); h->mat.d_ci_own = std::move(ci); h->mat.d_v_own = std::move(v);
    h->d_rp = h->mat.d_rp_own; h->d_ci = h->mat.d_ci_own; h->d_v = h->mat.d_v_own;
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
    h->M = M; h->K = K; h->nnz = nnz;
    free_dense(h);
    return SEXTANS_OK;
}

}  // extern "C"
namespace {
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
    if (h->cluster.state <= 0 || !h->cluster.d_slot_row || h->cluster.psc.plan_nblk <= 0) return SEXTANS_OK;
    const int RB = kBlock / 4 * std::max(1, h->cluster.psc.plan_sets);
    std::vector<int> sr((size_t)h->cluster.psc.plan_nblk * RB);
    SX_HIP(hipMemcpy(sr.data(), h->cluster.d_slot_row, sizeof(int) * sr.size(), hipMemcpyDeviceToHost));
    const std::vector<int> &br = h->cluster.psc.h_blk_row;
    if ((int)br.size() != h->cluster.psc.plan_nblk + 1) return SEXTANS_OK;
    int64_t in_runs = 0, slots = 0;
    for (int b = 0; b < h->cluster.psc.plan_nblk; ++b) {
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
    const sextans_engine::PanelState &P = h->cluster.state > 0 ? h->cluster.psc : h->ps;
    *value = 0.0;
    if (!P.plan_built || P.plan_nblk < 2 || !P.d_dict || !P.d_dict_ptr) return SEXTANS_OK;
    DevBuf<unsigned long long> d;
    unsigned long long hv[2] = {0, 0};
    SX_HIP(d.alloc(2));
    SX_HIP(hipMemset(d, 0, sizeof hv));
    hipLaunchKernelGGL(dict_overlap, dim3((unsigned)P.plan_nblk - 1), dim3(64), 0, hipStreamPerThread, P.d_dict_ptr, P.d_dict, P.plan_dict_stride, P.plan_nblk, d);
    SX_HIP(hipMemcpy(hv, d, sizeof hv, hipMemcpyDeviceToHost));
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
    if (!strcmp(key, "plan_build_s")) *value = h->mat.plan_build_s;
    else if (!strcmp(key, "window_padded_entries")) *value = (double)h->win.padded;
    else if (!strcmp(key, "window_state")) *value = (double)h->win.state;
    else if (!strcmp(key, "reassociated_rows")) *value = (double)h->split.h_split_rows.size();
    else if (!strcmp(key, "piece_path_rows")) *value = (double)(h->split.nhub + h->split.nchain);
    else if (!strcmp(key, "exact_chain_rows")) *value = (double)h->split.nchain;
    else if (!strcmp(key, "chain_threshold")) *value = (double)h->split.chain_T;
    else if (!strcmp(key, "split_threshold")) *value = (double)h->split.T;
    else if (!strcmp(key, "bucket_threshold")) *value = (double)h->split.bucket_L0;
    else if (!strcmp(key, "dense_tiles")) *value = (double)h->dense.tiles;
    else if (!strcmp(key, "dense_tile_fraction")) *value = h->nnz > 0 ? (double)h->dense.nnz / (double)h->nnz : 0.0;
    else if (!strcmp(key, "dense_tiles_on_mfma")) *value = h->dense.W > 0 ? 1.0 : 0.0;
    else if (!strcmp(key, "bell_share")) *value = h->bell_share;
    else if (!strcmp(key, "bell_variant")) *value = (double)h->bell_variant;   // 1 / 2 / 4 = spmm_bell_mfma<NSUB>, 8 = _n256, 9 = _shared, 0 = none yet
    else if (!strcmp(key, "row_cluster")) *value = (double)h->cluster.state;          // 1 grid bricks / 2 graph clustering in use, -1 declined, 0 not evaluated yet
    else if (!strcmp(key, "cluster_shared_fraction")) *value = h->cluster.shared;
    else if (!strcmp(key, "cluster_decline")) *value = (double)h->cluster.decline;
    else if (!strcmp(key, "graph_fallbacks")) *value = (double)h->graph_fallbacks;   // rp_time loops launched one by one because their hipGraph capture was invalidated from outside
    else if (!strcmp(key, "cluster_run16_fraction")) return run16_stat(h, value);   // share of the clustered plan's slots in runs of >= 16 consecutive rows of their block
    else if (!strcmp(key, "dict_overlap_consecutive")) return dict_overlap_stat(h, value);   // share of a block's dictionary rows the previous block of the walk holds too (the plan whole-matrix calls use)
    else if (!strcmp(key, "dist_setup_exchanges")) *value = (double)h->dist_exchanges;   // control collectives + host syncs of the dist entry points so far (0 new ones after sextans_dist_prepare)
    else if (!strcmp(key, "cluster_graph_kind")) *value = (double)h->cluster.graph_kind;
    else if (!strcmp(key, "cluster_runs")) *value = h->cluster.runs ? 1.0 : 0.0;
    else if (!strcmp(key, "pattern_symmetry")) *value = h->cluster.pattern_symmetry;
    else if (!strcmp(key, "col_range_lo")) *value = (double)h->col_lo;
    else if (!strcmp(key, "col_range_hi")) *value = (double)h->col_hi;
    else if (!strcmp(key, "b_rows_repacked")) *value = h->mat.d_touched ? (double)h->mat.touched_segments * 64.0 : (double)(h->col_hi - h->col_lo);
    else if (!strcmp(key, "colwise")) *value = (double)h->cluster.colwise_state;
    else if (!strcmp(key, "mixed_plan")) *value = h->ps.plan_built && h->ps.plan_mixed ? (h->ps.d_rg_skip && h->opt_split_mixed != 0 ? 2.0 : 1.0) : 0.0;   // 2: runs in its split form
    else if (!strcmp(key, "row_sets")) *value = (double)(h->cluster.state > 0 ? h->cluster.psc.plan_sets : h->ps.plan_sets);
    else if (!strcmp(key, "row_coherence")) *value = h->cluster.row_coherence;
    else if (!strcmp(key, "panel_blocks_clustered")) *value = (double)h->cluster.psc.plan_nblk;
    else if (!strcmp(key, "device_bytes")) *value = (double)device_bytes(h);
    else if (!strcmp(key, "softmax_long_rows")) *value = (double)h->softmax.long_rows;                  // rows on the long-row path of sextans_row_softmax*_device
    else if (!strcmp(key, "value_refreshes")) *value = (double)h->mat.value_refreshes;                  // sextans_update_values* served on this matrix
    else if (!strcmp(key, "value_refresh_rebuilt")) *value = (double)h->mat.value_refresh_rebuilt;      //   ... that dropped a form for a lazy rebuild
    else if (!strcmp(key, "bf16_native_calls")) *value = (double)(h->mat.bf16_native_calls + (h->tr ? h->tr->mat.bf16_native_calls : 0));            // bf16 calls (transposed ones included) on the caller's buffers
    else if (!strcmp(key, "bf16_converted_calls")) *value = (double)(h->mat.bf16_converted_calls + (h->tr ? h->tr->mat.bf16_converted_calls : 0));   //   ... and through fp32 copies
    else if (!strcmp(key, "transpose_build_s")) *value = h->at.build_s + (h->tr ? h->tr->mat.plan_build_s : 0.0);
    else if (!strcmp(key, "grid_stride_line")) *value = (double)h->cluster_s2;
    else if (!strcmp(key, "grid_stride_plane")) *value = (double)h->cluster_s3;
    else if (!strcmp(key, "panel_rows_natural")) *value = (double)h->plan_total_dict;  // B rows copied into LDS per N tile, natural order
    else if (!strcmp(key, "panel_rows_clustered")) *value = (double)h->cluster.total_dict;
    else if (!strcmp(key, "panel_fraction")) *value = h->ps.plan_panel_frac;
    else if (!strcmp(key, "panel_blocks")) *value = (double)h->ps.plan_nblk;
    else if (!strcmp(key, "index_stream_entries")) *value = (double)(h->cluster.state > 0 ? h->cluster.psc.plan_idx_len : h->ps.plan_idx_len);
    else if (!strcmp(key, "value_stream_entries")) *value = (double)(h->cluster.state > 0 ? h->cluster.psc.plan_stream_len : h->ps.plan_stream_len);
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
    const int M = h->M, nblk = ps.plan_nblk, RB = kBlock / lanes_per_row;
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
    *count = (int)h->split.h_split_rows.size();
    for (int i = 0; i < *count && i < capacity; ++i) rows[i] = h->split.h_split_rows[(size_t)i];
    return SEXTANS_OK;
}

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
    const bool have = h->cluster.state > 0 && h->cluster.d_slot_row && h->cluster.psc.plan_built && h->split.nhub == 0 && h->split.nchain == 0;
    if (clustered) *clustered = have ? h->cluster.state : 0;
    if (!have) {
        for (int i = 0; i < h->M; ++i) order[i] = i;
        return SEXTANS_OK;
    }
    DevBuf<int> d_tab;
    SX_HIP(d_tab.alloc((size_t)std::max(h->M, 1)));
    cc_table(h, 0, d_tab, nullptr);
    SX_HIP(hipMemcpy(order, d_tab, sizeof(int) * (size_t)h->M, hipMemcpyDeviceToHost));
    return SEXTANS_OK;
}

int sextans_profile_reset(sextans_handle_t h) {
    if (!h) return SEXTANS_ERR_INVALID;
    for (auto *vec : {&h->ev_kernel, &h->ev_repack, &h->ev_post}) {
        for (auto &ep : *vec) { (void)hipEventDestroy(ep.a); (void)hipEventDestroy(ep.b); }
        vec->clear();
    }
    return SEXTANS_OK;
}

static int mean_ns(std::vector<EventPair> &v, double *out) {   // mean time of the event pairs recorded (waits for them)
    double tot = 0.0;
    for (auto &ep : v) {
        SX_HIP(hipEventSynchronize(ep.b));
        float ms = 0.f;
        SX_HIP(hipEventElapsedTime(&ms, ep.a, ep.b));
        tot += (double)ms * 1e6;
    }
    if (out) *out = v.empty() ? 0.0 : tot / (double)v.size();
    return SEXTANS_OK;
}

int sextans_profile_read(sextans_handle_t h, double *mean_kernel_ns, int64_t *launches, double *mean_repack_ns) {
    if (!h) return SEXTANS_ERR_INVALID;
    SX_HIP(hipSetDevice(h->device));
    if (int rc = mean_ns(h->ev_kernel, mean_kernel_ns)) return rc;
    if (int rc = mean_ns(h->ev_repack, mean_repack_ns)) return rc;
    if (launches) *launches = (int64_t)h->ev_kernel.size();
    return SEXTANS_OK;
}

int sextans_profile_read_post(sextans_handle_t h, double *mean_post_ns, int64_t *launches) {
    if (!h) return SEXTANS_ERR_INVALID;
    SX_HIP(hipSetDevice(h->device));
    if (int rc = mean_ns(h->ev_post, mean_post_ns)) return rc;
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
