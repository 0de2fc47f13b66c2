// engine_gated.hip -- gated aggregation over the CSR pattern on an engine handle (include/sextans_amd.h):
//   sextans_spmm_gated_device_rm            C[r, :] = sum over row r's entries of sigmoid(xdst[r] + xsrc[c] (+ E[e])) * V[c], as it is (SUM) or
//                                           divided by the sum of the gates + eps (NORM); optionally the gates' sum and the pre-activations z
//   sextans_spmm_gated_workspace_floats     the floats of workspace the backward needs (NORM: gn = G / (den + eps), M x N; SUM: none), for
//                                           either element type
//   sextans_spmm_gated_backward_device_rm   dxdst and dE (a row pass over A), dxsrc and dV (a column pass over A^T), each only when asked for
// Kernels: spmm_gated_kernels.h on the row walking of pattern_pass.h; the entry points' frame: pattern_launch.h; the checks and the passes
// of both entry points: gated_launch.h, here for fp32 edge tensors (bf16: engine_gated_bf16.hip and engine_gated_bf16_backward.hip).  Only
// the pattern is read: neither the engine's values nor any of its packed forms is read or touched.
#include "gated_launch.h"

namespace sx {

// gn = G / (den + eps), M x N at leading dimension N: both backward passes read these bits
__global__ __launch_bounds__(256) void gated_gn(long long rows, int n4, const float *__restrict__ G, long long ldg, const float *__restrict__ den,
                                                long long ldden, float eps, float *__restrict__ gn) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * n4) return;
    const long long r = i / n4;
    const int c = 4 * (int)(i % n4);
    const float4 g = *reinterpret_cast<const float4 *>(G + r * ldg + c), d = *reinterpret_cast<const float4 *>(den + r * ldden + c);
    *reinterpret_cast<float4 *>(gn + r * (4LL * n4) + c) = make_float4(__fdiv_rn(g.x, __fadd_rn(d.x, eps)), __fdiv_rn(g.y, __fadd_rn(d.y, eps)),
                                                                        __fdiv_rn(g.z, __fadd_rn(d.z, eps)), __fdiv_rn(g.w, __fadd_rn(d.w, eps)));
}

}  // namespace sx

namespace sxe {

void gated_normalize(int64_t M, int N, const float *d_G, int64_t ldg, const float *d_den, int64_t ldden, float eps, float *d_gn, hipStream_t s) {
    const long long items = (long long)M * (N / 4);
    hipLaunchKernelGGL(sx::gated_gn, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, (long long)M, N / 4, d_G, (long long)ldg, d_den,
                       (long long)ldden, eps, d_gn);
}

}  // namespace sxe

using namespace sxe;

extern "C" {

int sextans_spmm_gated_device_rm(sextans_handle_t h, int mode, float eps, int N, const sextans_gated_in *in, float *d_C, int64_t ldc,
                                 float *d_den, int64_t ldden, float *d_z, int64_t ldz, void *stream) {
    return gated_forward<float>(h, mode, eps, N, in, d_C, ldc, d_den, ldden, d_z, ldz, stream, "spmm_gated");
}

int64_t sextans_spmm_gated_workspace_floats(sextans_handle_t h, int mode, int N) {
    if (!h || bad_mode(mode) || bad_n(N) || too_many_tiles(N, kMaxTile)) return -(int64_t)SEXTANS_ERR_INVALID;
    if (!h->d_rp) return -(int64_t)SEXTANS_ERR_STATE;
    return mode == SEXTANS_GATE_NORM ? (int64_t)h->M * N : 0;
}

int sextans_spmm_gated_backward_device_rm(sextans_handle_t h, int mode, float eps, int N, const sextans_gated_in *in, const float *d_C, int64_t ldc,
                                          const float *d_den, int64_t ldden, const float *d_G, int64_t ldg, const float *d_Gz, int64_t ldgz,
                                          const sextans_gated_grad *out, float *d_work, void *stream) {
    return gated_backward<float>(h, mode, eps, N, in, d_C, ldc, d_den, ldden, d_G, ldg, d_Gz, ldgz, out, d_work, stream, "spmm_gated_backward");
}

}  // extern "C"
