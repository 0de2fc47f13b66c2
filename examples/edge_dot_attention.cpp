// examples/edge_dot_attention.cpp -- u_dot_v -> edge_softmax -> u_mul_e_sum on a CSR pattern through the C ABI alone (no Python, no
// torch), captured into ONE hipGraph: the transformer-style layer a graph library writes with custom scores.
//
//   edge_dot_attention <A.mtx> [heads] [d]
//
// S[e, h] = <Q[r, h, :], K[c, h, :]> for every stored entry (sextans_edge_dot_device, all heads in one launch), then
// O[r, h, :] = sum_e softmax_e(S[:, h] over row r) V[c, h, :] (sextans_score_attention_device).  Anything elementwise on S -- a clamp, a
// temperature, an additive per-edge term -- would be one more node between the two.  After sextans_prepare(ROWMAJOR_T) neither call
// allocates or synchronises, so both are captured on one stream and replayed with new operand contents.  The result of the second
// replay is compared with a double-precision host computation; exit code 0 = it agrees to 1e-4.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sextans_amd.h"

#define CHECK(call)                                                                                  \
    do {                                                                                             \
        int rc_ = (call);                                                                            \
        if (rc_ != SEXTANS_OK) {                                                                     \
            fprintf(stderr, "%s: %s (%s)\n", #call, sextans_error_string(rc_), sextans_last_error()); \
            exit(2);                                                                                 \
        }                                                                                            \
    } while (0)
#define HIP(call) do { if ((call) != hipSuccess) { fprintf(stderr, "%s failed\n", #call); exit(2); } } while (0)

static void fill(std::vector<float> &x, unsigned seed) {
    for (auto &v : x) { seed = seed * 1664525u + 1013904223u; v = (float)(seed >> 8) / 8388608.0f - 1.0f; }
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <A.mtx> [heads] [d]\n", argv[0]); return 1; }
    const int H = argc > 2 ? atoi(argv[2]) : 4, d = argc > 3 ? atoi(argv[3]) : 16;
    int M, K, nnz, *rp, *ci;
    float *va;
    CHECK(sextans_mtx_read(argv[1], SEXTANS_FMT_CSR, &M, &K, &nnz, &rp, &ci, &va));
    sextans_handle_t h;
    CHECK(sextans_create(&h, 0));
    CHECK(sextans_set_matrix_csr(h, M, K, nnz, rp, ci, va));   // only the pattern is used below
    hipStream_t st;
    HIP(hipStreamCreate(&st));
    CHECK(sextans_prepare(h, H * d, SEXTANS_LAYOUT_ROWMAJOR_T, st));   // the row table, the passes' tables (and A^T for a backward)
    HIP(hipStreamSynchronize(st));

    const size_t nq = (size_t)M * H * d, nk = (size_t)K * H * d;
    std::vector<float> Q(nq), Kk(nk), V(nk), O(nq);
    float *dQ, *dK, *dV, *dS, *dO, *dlse;
    HIP(hipMalloc(&dQ, nq * 4)); HIP(hipMalloc(&dK, nk * 4)); HIP(hipMalloc(&dV, nk * 4)); HIP(hipMalloc(&dO, nq * 4));
    HIP(hipMalloc(&dS, (size_t)nnz * H * 4)); HIP(hipMalloc(&dlse, (size_t)M * H * 4));

    hipGraph_t graph;
    hipGraphExec_t exec;
    HIP(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    CHECK(sextans_edge_dot_device(h, H, d, dQ, H * d, dK, H * d, dS, H, st));
    CHECK(sextans_score_attention_device(h, SEXTANS_SCORE_SOFTMAX, H, d, dS, H, dV, H * d, dO, H * d, dlse, nullptr, st));
    HIP(hipStreamEndCapture(st, &graph));
    HIP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));

    for (unsigned step = 0; step < 2; ++step) {   // new contents, the same graph
        fill(Q, 1 + 3 * step); fill(Kk, 2 + 3 * step); fill(V, 3 + 3 * step);
        HIP(hipMemcpyAsync(dQ, Q.data(), nq * 4, hipMemcpyHostToDevice, st));
        HIP(hipMemcpyAsync(dK, Kk.data(), nk * 4, hipMemcpyHostToDevice, st));
        HIP(hipMemcpyAsync(dV, V.data(), nk * 4, hipMemcpyHostToDevice, st));
        HIP(hipGraphLaunch(exec, st));
        HIP(hipMemcpyAsync(O.data(), dO, nq * 4, hipMemcpyDeviceToHost, st));
        HIP(hipStreamSynchronize(st));
    }

    double worst = 0.0;
    std::vector<double> s, o(d);
    for (int r = 0; r < M; ++r) {
        for (int hd = 0; hd < H; ++hd) {
            const int b = rp[r], e = rp[r + 1];
            s.assign(e - b, 0.0);
            double mx = -INFINITY, z = 0.0;
            for (int j = b; j < e; ++j) {
                for (int n = 0; n < d; ++n) s[j - b] += (double)Q[((size_t)r * H + hd) * d + n] * Kk[((size_t)ci[j] * H + hd) * d + n];
                mx = std::fmax(mx, s[j - b]);
            }
            o.assign(d, 0.0);
            for (int j = b; j < e; ++j) {
                const double p = std::exp(s[j - b] - mx);
                z += p;
                for (int n = 0; n < d; ++n) o[n] += p * V[((size_t)ci[j] * H + hd) * d + n];
            }
            for (int n = 0; n < d; ++n)
                worst = std::fmax(worst, std::fabs((e > b ? o[n] / z : 0.0) - O[((size_t)r * H + hd) * d + n]));
        }
    }
    printf("edge_dot -> score_attention in one graph: %d x %d, %d entries, %d heads of %d; last kernel %s; max |O - host| = %.3g\n", M, K, nnz, H, d,
           sextans_last_kernel(h), worst);

    (void)hipGraphExecDestroy(exec); (void)hipGraphDestroy(graph);
    (void)hipFree(dQ); (void)hipFree(dK); (void)hipFree(dV); (void)hipFree(dS); (void)hipFree(dO); (void)hipFree(dlse);
    (void)hipStreamDestroy(st);
    sextans_destroy(h);
    sextans_host_free(rp); sextans_host_free(ci); sextans_host_free(va);
    return worst < 1e-4 ? 0 : 3;
}
