// engine_softmax.hip -- row softmax over the stored entries of the CSR matrix on an engine handle (include/sextans_amd.h):
//   sextans_row_softmax_device            p = softmax(scale * x) per row of A's pattern
//   sextans_row_softmax_backward_device   dx = scale * p * (g - sum_row p g)
// Kernels and the work split: row_softmax_kernels.h.  The tables depend on row_ptr alone: built once per matrix (first call or
// sextans_prepare(..., SEXTANS_LAYOUT_ROWMAJOR_T, ...)), untouched by value refreshes, dropped with the matrix (free_backward).
#include "engine_state.h"
#include "row_softmax_kernels.h"

namespace sxe {

void free_softmax(sextans_engine *h) {
    h->softmax = {};
}

int ensure_softmax_tables(sextans_engine *h, hipStream_t s) {
    if (h->softmax.d_sm_wrow || h->nnz == 0 || h->M == 0) return SEXTANS_OK;
    if (int rc = validate_matrix(h)) return rc;
    const int64_t nw = (h->nnz + sx::kSoftmaxWaveEntries - 1) / sx::kSoftmaxWaveEntries;
    DevBuf<int> d_wrow, d_cnt;   // d_cnt: long rows, their chunks, the fill cursor
    auto fail = [&](int rc, const char *what) {
        if (what) { g_last_error = what; (void)hipGetLastError(); }
        free_softmax(h);
        return rc;
    };
    if (d_wrow.alloc((size_t)(nw + 1)) != hipSuccess || d_cnt.alloc(4) != hipSuccess)
        return fail(SEXTANS_ERR_ALLOC, "row softmax: out of device memory for the wavefront table");
    int cnt[4] = {0, 0, 0, 0};
    const dim3 rows_grid((unsigned)(((int64_t)h->M + 255) / 256));
    if (hipMemsetAsync(d_cnt, 0, sizeof(int) * 4, s) != hipSuccess) return fail(SEXTANS_ERR_HIP, "row softmax: hipMemsetAsync failed");
    hipLaunchKernelGGL(sx::softmax_wave_rows, dim3((unsigned)((nw + 1 + 255) / 256)), dim3(256), 0, s, h->M, h->d_rp, (long long)nw, d_wrow);
    if (hipGetLastError() != hipSuccess) return fail(SEXTANS_ERR_HIP, "row softmax: launching softmax_wave_rows failed");
    hipLaunchKernelGGL(sx::softmax_count_long, rows_grid, dim3(256), 0, s, h->M, h->d_rp, d_cnt);
    if (hipGetLastError() != hipSuccess) return fail(SEXTANS_ERR_HIP, "row softmax: launching softmax_count_long failed");
    if (hipMemcpyAsync(cnt, d_cnt, sizeof(int) * 2, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return fail(SEXTANS_ERR_HIP, "row softmax: counting the long rows failed");
    if (cnt[1] > 0) {
        if (h->softmax.d_sm_tab.alloc((size_t)cnt[1]) != hipSuccess ||
            h->softmax.d_sm_part.alloc(2 * (size_t)cnt[1]) != hipSuccess)   // partials + per-row results
            return fail(SEXTANS_ERR_ALLOC, "row softmax: out of device memory for the long-row tables");
        hipLaunchKernelGGL(sx::softmax_fill_long, rows_grid, dim3(256), 0, s, h->M, h->d_rp, d_cnt + 2, cnt[1], h->softmax.d_sm_tab);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return fail(SEXTANS_ERR_HIP, "row softmax: building the long-row table failed");
    }
    d_cnt.reset();
    h->softmax.d_sm_wrow = std::move(d_wrow);
    h->softmax.long_rows = cnt[0];
    h->softmax.nchunks = cnt[1];
    return SEXTANS_OK;
}

namespace {

int check_args(sextans_handle_t h, const void *a, const void *b, const void *c) {   // nothing here needs a device
    if (!h) return SEXTANS_ERR_INVALID;
    if (((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) != 0) return SEXTANS_ERR_INVALID;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    if (h->nnz > 0 && (!a || !b || !c)) return SEXTANS_ERR_INVALID;
    return SEXTANS_OK;
}

template <bool BWD>
int run(sextans_engine *h, float scale, const float *x, const float *g, float *out, hipStream_t s) {
    SX_HIP(hipSetDevice(h->device));
    if (h->nnz == 0 || h->M == 0) return SEXTANS_OK;
    if (int rc = ensure_softmax_tables(h, s)) return rc;
    const long long nw = (long long)h->softmax.d_sm_wrow.size() - 1;
    const int nnz = (int)h->nnz;
    hipLaunchKernelGGL((sx::row_softmax_rows<BWD>), dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, s, nnz, h->d_rp, h->softmax.d_sm_wrow, nw, scale, x, g, out);
    SX_HIP(hipGetLastError());
    if (h->softmax.nchunks > 0) {
        const dim3 grid((unsigned)((h->softmax.nchunks + 3) / 4));
        float2 *part = h->softmax.d_sm_part, *res = h->softmax.d_sm_part + h->softmax.nchunks;
        hipLaunchKernelGGL((sx::softmax_long_partial<BWD>), grid, dim3(256), 0, s, nnz, h->d_rp, h->softmax.d_sm_tab, h->softmax.nchunks, scale, x, g, part);
        hipLaunchKernelGGL((sx::softmax_long_combine<BWD>), grid, dim3(256), 0, s, h->d_rp, h->softmax.d_sm_tab, h->softmax.nchunks, part, res);
        hipLaunchKernelGGL((sx::softmax_long_finish<BWD>), grid, dim3(256), 0, s, nnz, h->d_rp, h->softmax.d_sm_tab, h->softmax.nchunks, scale, x, g, res, out);
        SX_HIP(hipGetLastError());
    }
    h->last_kernel = BWD ? (h->softmax.nchunks > 0 ? "row_softmax_backward+long_rows" : "row_softmax_backward")
                         : (h->softmax.nchunks > 0 ? "row_softmax+long_rows" : "row_softmax");
    return SEXTANS_OK;
}

}  // namespace
}  // namespace sxe

using namespace sxe;

extern "C" {

int sextans_row_softmax_device(sextans_handle_t h, float scale, const float *d_x, float *d_p, void *stream) {
    if (int rc = check_args(h, d_x, d_p, d_p)) return rc;
    return run<false>(h, scale, d_x, nullptr, d_p, (hipStream_t)stream);
}

int sextans_row_softmax_backward_device(sextans_handle_t h, float scale, const float *d_p, const float *d_g, float *d_dx, void *stream) {
    if (int rc = check_args(h, d_p, d_g, d_dx)) return rc;
    return run<true>(h, scale, d_p, d_g, d_dx, (hipStream_t)stream);
}

}  // extern "C"
