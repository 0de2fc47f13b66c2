// csr_transpose.hip -- stable transpose of a device-resident CSR matrix (csr_transpose.h) and its C entry point.
//
// expand   row id of every entry (one wavefront per row);
// sort     (column, entry index) pairs, hipcub's stable LSD radix sort over bits(K) key bits: inside a column the entries keep their
//          CSR order, i.e. ascending row and, for duplicates, storage order -- CSC_2_CSR's traversal (sparse_helper.h:475-509);
// gather   row id and value of each sorted entry (the pattern alone: the row ids are the sort's values, no gather);
// starts   row pointer of A^T by binary search of every column in the sorted keys.
// Every position follows from the sort alone: no atomics, the same bits on every run.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <vector>

#include "csr_transpose.h"
#include "plan_device.h"
#include "sextans_amd.h"
#include "thread_stream.h"

namespace sx {
namespace {

#define TR_HIP(x)                                                                                       \
    do {                                                                                                \
        hipError_t e_ = (x);                                                                            \
        if (e_ != hipSuccess) { err = std::string(#x) + ": " + hipGetErrorString(e_); return 2; }       \
    } while (0)

struct SyncOnExit {   // declared behind the scratch buffers of a function: nothing enqueued may still read them when they are freed
    hipStream_t s;
    ~SyncOnExit() { (void)hipStreamSynchronize(s); }
};

inline unsigned blocks_for(long long n, int per) { return (unsigned)((n + per - 1) / per); }

__global__ __launch_bounds__(256) void expand_row_ids(int M, const int *__restrict__ rp, int *__restrict__ rows) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + wave;
    if (r >= M) return;
    for (int j = rp[r] + lane; j < rp[r + 1]; j += 64) rows[j] = r;
}
__global__ __launch_bounds__(256) void iota(long long n, int *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (int)i;
}
__global__ __launch_bounds__(256) void column_starts(int K, long long nnz, const int *__restrict__ sorted_cols, int *__restrict__ cp) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c > K) return;
    long long lo = 0, hi = nnz;                     // first position whose column is >= c
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if (sorted_cols[mid] < c) lo = mid + 1; else hi = mid; }
    cp[c] = (int)lo;
}
__global__ __launch_bounds__(256) void gather_entries(long long nnz, const int *__restrict__ seid, const int *__restrict__ rows,
                                                      const float *__restrict__ v, int *__restrict__ t_ci, float *__restrict__ t_v) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nnz) return;
    const int e = seid[i];
    t_ci[i] = rows[e];
    t_v[i] = v[e];
}

}  // namespace

void segment_starts_device(int n, int64_t nnz, const int *sorted, int *starts, hipStream_t s) {
    hipLaunchKernelGGL(column_starts, dim3(blocks_for((long long)n + 1, 256)), dim3(256), 0, s, n, (long long)nnz, sorted, starts);
}

int csr_transpose_device(int M, int K, int64_t nnz, const int *d_rp, const int *d_ci, const float *d_v, int *t_rp, int *t_ci, float *t_v,
                         hipStream_t s, std::string &err, int *t_perm) {
    if (nnz <= 0) {   // every row of A^T is empty
        TR_HIP(hipMemsetAsync(t_rp, 0, sizeof(int) * ((size_t)K + 1), s));
        TR_HIP(hipStreamSynchronize(s));
        return 0;
    }
    DevBuf<int> rows, scols, eid, seid_own;
    DevBuf<char> sort_tmp;
    SyncOnExit sync{s};
    TR_HIP(rows.alloc((size_t)nnz));
    TR_HIP(scols.alloc((size_t)nnz));
    hipLaunchKernelGGL(expand_row_ids, dim3(blocks_for(M, 4)), dim3(256), 0, s, M, d_rp, rows);
    int bits = 1;
    while (bits < 32 && (1LL << bits) < (long long)K) ++bits;
    size_t bytes = 0;
    if (!d_v) {   // the pattern alone (the row-similarity graph): the row ids travel through the sort straight into t_ci
        TR_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, d_ci, scols.get(), rows.get(), t_ci, (int)nnz, 0, bits, s));
        TR_HIP(sort_tmp.alloc(bytes));
        TR_HIP(hipcub::DeviceRadixSort::SortPairs(sort_tmp.get(), bytes, d_ci, scols.get(), rows.get(), t_ci, (int)nnz, 0, bits, s));   // stable: rows ascending per column
    } else {      // values too: the entry index travels through the sort, row id and value are gathered behind it
        TR_HIP(eid.alloc((size_t)nnz));
        if (!t_perm) TR_HIP(seid_own.alloc((size_t)nnz));
        int *seid = t_perm ? t_perm : seid_own.get();   // the caller keeps the sorted entry indices: t_v[i] = d_v[t_perm[i]] for every later set of values
        hipLaunchKernelGGL(iota, dim3(blocks_for(nnz, 256)), dim3(256), 0, s, (long long)nnz, eid);
        TR_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, d_ci, scols.get(), eid.get(), seid, (int)nnz, 0, bits, s));
        TR_HIP(sort_tmp.alloc(bytes));
        TR_HIP(hipcub::DeviceRadixSort::SortPairs(sort_tmp.get(), bytes, d_ci, scols.get(), eid.get(), seid, (int)nnz, 0, bits, s));   // stable: CSR order per column
        hipLaunchKernelGGL(gather_entries, dim3(blocks_for(nnz, 256)), dim3(256), 0, s, (long long)nnz, seid, rows, d_v, t_ci, t_v);
    }
    segment_starts_device(K, nnz, scols, t_rp, s);
    TR_HIP(hipGetLastError());
    TR_HIP(hipStreamSynchronize(s));
    return 0;
}

}  // namespace sx

extern "C" int sextans_csr_transpose_device(int device, int M, int K, int64_t nnz, const int *d_row_ptr, const int *d_col_idx,
                                            const float *d_val, int **o_row_ptr, int **o_col_idx, float **o_val, void *stream) {
    if (M < 0 || K < 0 || nnz < 0 || nnz > 0x7fffffffLL || (M == 0 && nnz > 0) || !d_row_ptr || (nnz > 0 && (!d_col_idx || !d_val)) ||
        !o_row_ptr || !o_col_idx || !o_val)
        return SEXTANS_ERR_INVALID;
    *o_row_ptr = *o_col_idx = nullptr;
    *o_val = nullptr;
    if (hipSetDevice(device) != hipSuccess) return SEXTANS_ERR_NO_DEVICE;
    std::string err;
    {   // a public entry point: columns index the row pointer of A^T, so they must lie in [0, K)
        int bad = 0;
        if (M > 0 && sx::validate_csr_device(M, K, nnz, d_row_ptr, d_col_idx, &bad, err)) return SEXTANS_ERR_HIP;
        if (bad) return (bad & 1) ? SEXTANS_ERR_INVALID : SEXTANS_ERR_INDEX;
    }
    // (the arrays are the caller's from here on, to be released with sextans_device_free: raw memory like sextans_device_alloc's)
    int *trp = nullptr, *tci = nullptr;
    float *tv = nullptr;
    auto fail = [&](int rc) { (void)sextans_device_free(device, trp); (void)sextans_device_free(device, tci); (void)sextans_device_free(device, tv); return rc; };
    if (sextans_device_alloc(device, sizeof(int) * ((size_t)K + 1), (void **)&trp) != SEXTANS_OK ||
        sextans_device_alloc(device, sizeof(int) * (size_t)std::max<int64_t>(nnz, 1), (void **)&tci) != SEXTANS_OK ||
        sextans_device_alloc(device, sizeof(float) * (size_t)std::max<int64_t>(nnz, 1), (void **)&tv) != SEXTANS_OK)
        return fail(SEXTANS_ERR_ALLOC);
    if (sx::csr_transpose_device(M, K, nnz, d_row_ptr, d_col_idx, d_val, trp, tci, tv, (hipStream_t)stream, err)) return fail(SEXTANS_ERR_HIP);
    *o_row_ptr = trp; *o_col_idx = tci; *o_val = tv;
    return SEXTANS_OK;
}
