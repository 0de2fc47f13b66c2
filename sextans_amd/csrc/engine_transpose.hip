// engine_transpose.hip -- the two products of a backward pass on an engine handle (include/sextans_amd.h):
//   sextans_spmm_t_device_rm   alpha * A^T * B + beta * C_in through a companion engine that holds A^T (csr_transpose.hip), so that A^T
//                              gets every path of the dispatcher; no atomic scatter (run-to-run reproducible, strict mode bit-exact);
//   sextans_sddmm_device_rm    alpha * (X Y^T) sampled on A's pattern (sddmm_kernel.h).
#include <algorithm>
#include <chrono>

#include "csr_transpose.h"
#include "engine_state.h"
#include "plan_device.h"
#include "sddmm_kernel.h"

namespace sxe {

void free_transpose(sextans_engine *h) {
    if (h->tr) sextans_destroy(h->tr);
    h->tr = nullptr;
    h->at = {};
}

void free_backward(sextans_engine *h) {
    free_transpose(h);
    h->d_sddmm_row0 = {};
    free_softmax(h);
}

int validate_matrix(sextans_engine *h) {   // a device matrix nobody has looked at yet: its indices address X / Y rows and A^T's row pointer
    if (h->owns_matrix() || h->mat.device_matrix_checked || h->M == 0) return SEXTANS_OK;
    int bad = 0;
    std::string verr;
    if (sx::validate_csr_device(h->M, h->K, h->nnz, h->d_rp, h->d_ci, &bad, verr)) { g_last_error = verr; return SEXTANS_ERR_HIP; }
    if (bad) return (bad & 1) ? SEXTANS_ERR_INVALID : SEXTANS_ERR_INDEX;
    h->mat.device_matrix_checked = true;
    return SEXTANS_OK;
}

// A^T and its companion engine, once per matrix (the values are those of this moment; sextans_update_values* brings newer ones through d_tperm)
int ensure_transpose(sextans_engine *h, hipStream_t s) {
    if (h->tr) return SEXTANS_OK;
    const auto t0 = std::chrono::steady_clock::now();
    if (int rc = validate_matrix(h)) return rc;
    const size_t entries = (size_t)std::max<int64_t>(h->nnz, 1);
    if (h->at.d_trp.alloc((size_t)h->K + 1) != hipSuccess || h->at.d_tci.alloc(entries) != hipSuccess || h->at.d_tv.alloc(entries) != hipSuccess ||
        h->at.d_tperm.alloc(entries) != hipSuccess) {
        g_last_error = "transposed form: out of device memory for A^T";
        (void)hipGetLastError();
        free_transpose(h);   // (whatever was allocated before the failure)
        return SEXTANS_ERR_ALLOC;
    }
    std::string err;
    if (sx::csr_transpose_device(h->M, h->K, h->nnz, h->d_rp, h->d_ci, h->d_v, h->at.d_trp, h->at.d_tci, h->at.d_tv, s, err, h->at.d_tperm)) {
        g_last_error = err;
        free_transpose(h);
        return SEXTANS_ERR_HIP;
    }
    sextans_engine *tr = nullptr;
    if (int rc = sextans_create(&tr, h->device)) { free_transpose(h); return rc; }
    h->tr = tr;
    int rc = transposed_options(h, nullptr, 0);
    if (!rc) rc = sextans_set_matrix_csr_device(tr, h->K, h->M, h->nnz, h->at.d_trp, h->at.d_tci, h->at.d_tv);
    if (rc) { free_transpose(h); return rc; }
    tr->mat.device_matrix_checked = true;   // (built from a validated matrix)
    h->at.build_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return SEXTANS_OK;
}

// The row of the first entry of every wavefront range of the SDDMM kernel, once per matrix (engine_edge_dot.hip's forward walks the same
// ranges through the same table): the kernel reads two ints per wavefront instead of searching row_ptr (a 64-ary search per wavefront made 2 scattered row_ptr requests per entry: 4x the L2 requests of the
// row-group gather kernel on the FEM, profiles/train_step_pmc_fem_N16.txt)
int ensure_sddmm_rows(sextans_engine *h, hipStream_t s) {
    if (h->d_sddmm_row0 || h->nnz == 0) return SEXTANS_OK;
    if (int rc = validate_matrix(h)) return rc;
    const int64_t nw = (h->nnz + sx::kSddmmWaveEntries - 1) / sx::kSddmmWaveEntries;
    if (h->d_sddmm_row0.alloc((size_t)(nw + 1)) != hipSuccess) {
        (void)hipGetLastError();
        g_last_error = "sddmm: out of device memory for the row table";
        return SEXTANS_ERR_ALLOC;
    }
    hipLaunchKernelGGL(sx::sddmm_wave_rows, dim3((unsigned)((nw + 1 + 255) / 256)), dim3(256), 0, s, h->M, (long long)h->nnz, h->d_rp,
                       (long long)nw, h->d_sddmm_row0);
    SX_HIP(hipGetLastError());
    return SEXTANS_OK;
}

int prepare_transposed(sextans_engine *h, int N, hipStream_t s) {
    if (int rc = ensure_sddmm_rows(h, s)) return rc;
    if (int rc = ensure_softmax_tables(h, s)) return rc;
    SX_HIP(hipStreamSynchronize(s));
    if (h->K == 0) return SEXTANS_OK;
    if (int rc = ensure_transpose(h, s)) return rc;
    if (int rc = ensure_softmax_tables(h->tr, s)) return rc;   // the column pass of sextans_attention_backward_device walks A^T's rows
    return sextans_prepare(h->tr, N, SEXTANS_LAYOUT_ROWMAJOR, s);
}

template <int LPR, int NCH>
void launch_sddmm_nch(dim3 grid, hipStream_t s, const sextans_engine *h, int N, float alpha, const float *X, int64_t ldx, const float *Y,
                      int64_t ldy, float beta, const float *vin, float *vout) {
    hipLaunchKernelGGL((sx::sddmm_rowmajor<LPR, NCH>), grid, dim3(256), 0, s, (long long)h->nnz, h->d_rp, h->d_ci, h->d_sddmm_row0, N, alpha, X,
                       (long long)ldx, Y, (long long)ldy, beta, vin, vout);
}
template <int LPR>
void launch_sddmm(int nch_cap, dim3 grid, hipStream_t s, const sextans_engine *h, int N, float alpha, const float *X, int64_t ldx,
                  const float *Y, int64_t ldy, float beta, const float *vin, float *vout) {
    switch (nch_cap) {
    case 1: launch_sddmm_nch<LPR, 1>(grid, s, h, N, alpha, X, ldx, Y, ldy, beta, vin, vout); break;
    case 2: launch_sddmm_nch<LPR, 2>(grid, s, h, N, alpha, X, ldx, Y, ldy, beta, vin, vout); break;
    case 4: launch_sddmm_nch<LPR, 4>(grid, s, h, N, alpha, X, ldx, Y, ldy, beta, vin, vout); break;
    case 8: launch_sddmm_nch<LPR, 8>(grid, s, h, N, alpha, X, ldx, Y, ldy, beta, vin, vout); break;
    default: launch_sddmm_nch<LPR, 0>(grid, s, h, N, alpha, X, ldx, Y, ldy, beta, vin, vout); break;
    }
}

}  // namespace sxe

using namespace sxe;

extern "C" {

int sextans_spmm_t_device_rm(sextans_handle_t h, int N, float alpha, const float *d_B, int64_t ldb, float beta, const float *d_C_in,
                             int64_t ldc_in, float *d_C_out, int64_t ldc, void *stream) {
    if (!h || N <= 0 || (N % 8) != 0 || !d_B || !d_C_in || !d_C_out || ldb < N || ldc_in < N || ldc < N) return SEXTANS_ERR_INVALID;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    SX_HIP(hipSetDevice(h->device));
    if (h->K == 0) return SEXTANS_OK;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = ensure_transpose(h, s)) return rc;
    const int rc = sextans_spmm_device_rm(h->tr, N, alpha, d_B, ldb, beta, d_C_in, ldc_in, d_C_out, ldc, stream);
    h->last_kernel_buf = h->tr->last_kernel;   // (the companion's name may live in its own buffer)
    h->last_kernel = h->last_kernel_buf.c_str();
    return rc;
}

int sextans_spmm_t_device_rm_bf16(sextans_handle_t h, int N, float alpha, const uint16_t *d_B, int64_t ldb, float beta, const void *d_C_in,
                                  int64_t ldc_in, void *d_C_out, int64_t ldc, int c_dtype, void *stream) {
    if (int rc = check_rm_bf16_args(h, N, d_B, ldb, d_C_in, ldc_in, d_C_out, ldc, c_dtype)) return rc;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    SX_HIP(hipSetDevice(h->device));
    if (h->K == 0) return SEXTANS_OK;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = ensure_transpose(h, s)) return rc;
    const int rc = sextans_spmm_device_rm_bf16(h->tr, N, alpha, d_B, ldb, beta, d_C_in, ldc_in, d_C_out, ldc, c_dtype, stream);
    h->last_kernel_buf = h->tr->last_kernel;
    h->last_kernel = h->last_kernel_buf.c_str();
    return rc;
}

int sextans_sddmm_device_rm(sextans_handle_t h, int N, float alpha, const float *d_X, int64_t ldx, const float *d_Y, int64_t ldy, float beta,
                            const float *d_vals_in, float *d_vals_out, void *stream) {
    if (!h || N <= 0 || (N % 8) != 0 || !d_X || !d_Y || !d_vals_out || ldx < N || ldy < N || (ldx % 4) != 0 || (ldy % 4) != 0)
        return SEXTANS_ERR_INVALID;
    if (((reinterpret_cast<uintptr_t>(d_X) | reinterpret_cast<uintptr_t>(d_Y) | reinterpret_cast<uintptr_t>(d_vals_in) |
          reinterpret_cast<uintptr_t>(d_vals_out)) & 15) != 0)
        return SEXTANS_ERR_INVALID;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    SX_HIP(hipSetDevice(h->device));
    if (h->nnz == 0) return SEXTANS_OK;
    hipStream_t s = (hipStream_t)stream;
    if (int rc = ensure_sddmm_rows(h, s)) return rc;
    const long long waves = (h->nnz + sx::kSddmmWaveEntries - 1) / sx::kSddmmWaveEntries;
    const dim3 grid((unsigned)((waves + 3) / 4));
    // 4 lanes per entry (a 64-byte Y segment per request, 16 entries per wavefront in flight, the partial sum carried across chunks of 16
    // columns), 2 where 16 does not divide N; the X row is kept in registers up to 8 chunks
    const int lpr = (N / 4) % 4 == 0 ? 4 : 2;
    const int nch = N / (4 * lpr);
    const int nch_cap = nch <= 1 ? 1 : nch <= 2 ? 2 : nch <= 4 ? 4 : nch <= 8 ? 8 : 0;
    if (lpr == 4) launch_sddmm<4>(nch_cap, grid, s, h, N, alpha, d_X, ldx, d_Y, ldy, beta, d_vals_in, d_vals_out);
    else launch_sddmm<2>(nch_cap, grid, s, h, N, alpha, d_X, ldx, d_Y, ldy, beta, d_vals_in, d_vals_out);
    h->last_kernel = lpr == 4 ? "sddmm_rowmajor_lpr4" : "sddmm_rowmajor_lpr2";
    SX_HIP(hipGetLastError());
    return SEXTANS_OK;
}

}  // extern "C"
