// engine_host.hip -- the host-buffer and reference-shaped entry points: sextans_spmm_host, sextans_invoke (the accelerator's channel
// layouts and packed edge lists, sextans-host.cpp:237-251), sextans_spmm_csr.  All of them time rp_time repeats of the device entry.
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "engine_launch.h"

using namespace sxe;

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
            if (int rc = sextans_spmm_device_rows(h, N, alpha, h->d_B, h->K, beta, h->d_Cin, h->M, h->d_Cout, h->M, 0, h->M, (r ? SEXTANS_ROWS_REUSE_B_PANELS : 0) | nofuse, (void *)cs))
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
// column-major B, C_in and C_out of the host-buffer entry points
int ensure_staging(sextans_engine *h, size_t nB, size_t nC) {
    if (int rc = reserve(h->d_B, nB)) return rc;
    if (int rc = reserve(h->d_Cin, nC)) return rc;
    return reserve(h->d_Cout, nC);
}
}  // namespace
extern "C" {

int sextans_spmm_host(sextans_handle_t h, int N, float alpha, const float *B, float beta, float *C, int rp_time, double *elapsed_ns) {
    if (!h || !B || !C || N <= 0 || (N % 8) != 0) return SEXTANS_ERR_INVALID;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    if (rp_time < 1) rp_time = 1;
    SX_HIP(hipSetDevice(h->device));
    const size_t nB = (size_t)h->K * (size_t)N, nC = (size_t)h->M * (size_t)N;
    if (int rc = ensure_staging(h, nB, nC)) return rc;
    SX_HIP(hipMemcpy(h->d_B, B, nB * sizeof(float), hipMemcpyHostToDevice));
    SX_HIP(hipMemcpy(h->d_Cin, C, nC * sizeof(float), hipMemcpyHostToDevice));
    if (int rc = prepare(h, N)) return rc;   // allocations and the one-time packing of A stay outside the timed region
    double ns = 0.0;
    if (int rc = run_repeats(h, N, alpha, beta, rp_time, nullptr, nullptr, &ns)) return rc;
    if (elapsed_ns) *elapsed_ns = ns;
    SX_HIP(hipMemcpy(C, h->d_Cout, nC * sizeof(float), hipMemcpyDeviceToHost));
    return SEXTANS_OK;
}

int sextans_set_matrix_edges(sextans_handle_t h, const int32_t *edge_list_ptr, const uint64_t *const *edge_list_ch, int NUM_ITE, int NUM_A_LEN, int M, int K) {
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

int sextans_invoke(sextans_handle_t h, const int32_t *edge_list_ptr, const uint64_t *const *edge_list_ch, const float *const *mat_B_ch, int num_ch_b, const float *const *mat_C_ch_in,
                   float *const *mat_C_ch, int NUM_ITE, int NUM_A_LEN, int M, int K, int P_N, int alpha_u, int beta_u, double *elapsed_ns) {
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
    if (int rc = reserve(h->d_chB, (size_t)b_len * num_ch_b)) return rc;
    if (int rc = reserve(h->d_chC, (size_t)c_len * 8)) return rc;
    if (int rc = ensure_staging(h, nB, nC)) return rc;
    for (int c = 0; c < num_ch_b; ++c) {
        if (!mat_B_ch[c]) return SEXTANS_ERR_INVALID;
        SX_HIP(hipMemcpy(h->d_chB + (size_t)c * b_len, mat_B_ch[c], sizeof(float) * (size_t)b_used, hipMemcpyHostToDevice));
    }
    for (int c = 0; c < 8; ++c) {
        if (!mat_C_ch_in[c] || !mat_C_ch[c]) return SEXTANS_ERR_INVALID;
        SX_HIP(hipMemcpy(h->d_chC + (size_t)c * c_len, mat_C_ch_in[c], sizeof(float) * (size_t)c_used, hipMemcpyHostToDevice));
    }
    if (int rc = prepare(h, N)) return rc;
    const float pad = alpha * 0.0f + beta * 0.0f;    // what the accelerator writes into rows M .. colsize-1
    auto pre = [&](hipStream_t cs) {
        launch_chan_unpack_b(h->d_chB, b_len, b_cs, num_ch_b, K, N, h->d_B, cs);
        launch_chan_unpack_c(h->d_chC, c_len, c_cs, M, N, h->d_Cin, cs);
    };
    auto post = [&](hipStream_t cs) { launch_chan_pack_c(h->d_Cout, M, N, c_len, c_cs, pad, h->d_chC, cs); };
    double ns = 0.0;
    if (M > 0) {
        if (int rc = run_repeats(h, N, alpha, beta, rp_time, pre, post, &ns)) return rc;
    } else {
        pre(nullptr); post(nullptr);
        SX_HIP(hipDeviceSynchronize());
    }
    if (elapsed_ns) *elapsed_ns = ns;
    for (int c = 0; c < 8; ++c)
        SX_HIP(hipMemcpy(mat_C_ch[c], h->d_chC + (size_t)c * c_len, sizeof(float) * (size_t)c_used, hipMemcpyDeviceToHost));
    return SEXTANS_OK;
}

int sextans_spmm_csr(int M, int N, int K, int NNZ, float ALPHA, const int *CSRRowPtr, const int *CSRColIndex, const float *CSRVal, const float *mat_B, float BETA, float *mat_C) {
    sextans_handle_t h = nullptr;
    if (int rc = sextans_create(&h, 0)) return rc;
    int rc = sextans_set_matrix_csr(h, M, K, NNZ, CSRRowPtr, CSRColIndex, CSRVal);
    if (!rc) rc = sextans_spmm_host(h, N, ALPHA, mat_B, BETA, mat_C, 1, nullptr);
    sextans_destroy(h);
    return rc;
}

}  // extern "C"
