// engine_refresh.hip -- sextans_update_values*: new values for the pattern that is set, without planning again.
//
// Planning is a function of the pattern and the options alone (thresholds come from row lengths and nnz, dense-tile detection counts
// positions, explicit zeros are kept), so every packed form keeps its layout and only its copy of the values is rewritten, on the
// caller's stream, by the kernels of value_refresh_kernels.h -- the "numeric phase" next to the "analysis phase" of sextans_set_matrix_*
// + sextans_prepare.  After the call every form holds the bytes a fresh engine would have built from the new values.
//   rewritten (nothing allocated, nothing read back, no synchronisation: may be captured into a hipGraph):
//       the packed streams of the natural-order plan (every lanes_per_row: the active one and the parked ones), of the clustered plan
//       (grid bricks / graph clustering), the compacted main matrix behind the long-row split, the relabelled chain copy of the
//       reordered form, A^T and -- through this same entry point -- every form of its companion engine;
//   nothing to do: forms that read the live array (gather, lane-per-row, piece and natural chain paths) and a released natural stream
//       (restore_plan_streams rebuilds it from the live values);
//   dropped for a lazy rebuild (stat "value_refresh_rebuilt"): the window stream, and with dense tiles / routed row blocks on the matrix
//       cores everything downstream of the matrix as set (their side matrices hold rounded or re-ordered values, and the source matrix
//       is then an owned copy built on the host).
#include "engine_state.h"
#include "spmm_csr_kernels.h"
#include "value_refresh_kernels.h"

namespace sxe {
namespace {

void refresh_plan(const sextans_engine *h, const sextans_engine::PanelState &p, const int *slot_row, hipStream_t s) {
    if (!p.plan_built || p.stream_released || !p.d_pval || !p.plan_lpr || p.plan_nblk <= 0) return;
    const int slots = (sx::kBlock / p.plan_lpr) * p.plan_sets;
    hipLaunchKernelGGL(sx::refresh_packed_stream, dim3((unsigned)p.plan_nblk), dim3(256), 0, s, p.plan_nblk, slots, p.plan_lpr, p.d_blk_row, slot_row,
                       (const int2 *)p.d_row_off.get(), h->m_rp, (const unsigned *)h->m_v, (unsigned *)p.d_pval.get());
}

int refresh_forms(sextans_engine *h, hipStream_t s) {
    bool rebuilt = false;
    if (h->win.d_wstream) { free_window(h); rebuilt = true; }
    if (h->dense.d_sv || h->dense.W > 0 || h->dense.rb_n > 0) {   // dense tiles / row blocks were cut out: the source is an owned copy, the side matrices hold values
        free_plan(h);
        free_window(h);
        free_dense(h);
        rebuilt = true;
    }
    // the stages that alias the matrix as set follow its value array
    if (!h->dense.d_sv) h->s_v = h->d_v;
    if (!h->split.d_mv) h->m_v = h->s_v;
    if (h->split.d_mv && h->split.d_skip && h->M > 0)
        hipLaunchKernelGGL(sx::refresh_main_values, dim3((unsigned)((h->M + 3) / 4)), dim3(256), 0, s, h->M, h->s_rp, (const unsigned *)h->s_v,
                           (const unsigned char *)h->split.d_skip.get(), (const int *)h->split.d_mrp.get(), (unsigned *)h->split.d_mv.get());
    refresh_plan(h, h->ps, nullptr, s);
    for (const auto &p : h->plan_stash) refresh_plan(h, p, nullptr, s);
    refresh_plan(h, h->cluster.psc, h->cluster.d_slot_row, s);
    if (h->cluster.d_chain_v_c && h->split.nchain > 0)
        hipLaunchKernelGGL(sx::refresh_chain_values, dim3((unsigned)h->split.nchain), dim3(256), 0, s, h->split.d_chain_beg, h->split.d_chain_off, (const unsigned *)h->s_v,
                           (unsigned *)h->cluster.d_chain_v_c.get());
    if (h->tr) {   // (ensure_transpose allocates the entry permutation together with A^T)
        hipLaunchKernelGGL(sx::refresh_transposed, dim3((unsigned)((h->nnz + 255) / 256)), dim3(256), 0, s, (long long)h->nnz, h->at.d_tperm,
                           (const unsigned *)h->d_v, (unsigned *)h->at.d_tv.get());
        if (int rc = sextans_update_values_device(h->tr, h->at.d_tv, s)) return rc;
    }
    SX_HIP(hipGetLastError());
    ++h->mat.value_refreshes;
    if (rebuilt) ++h->mat.value_refresh_rebuilt;
    return SEXTANS_OK;
}

}  // namespace
}  // namespace sxe

using namespace sxe;

extern "C" {

int sextans_update_values_device(sextans_handle_t h, const float *d_val, void *stream) {
    if (!h) return SEXTANS_ERR_INVALID;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    if (h->nnz == 0) return SEXTANS_OK;
    if (!d_val) return SEXTANS_ERR_INVALID;
    SX_HIP(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (h->owns_matrix()) {   // the engine's own array keeps the values
        if (d_val != h->d_v) SX_HIP(hipMemcpyAsync((void *)h->d_v, d_val, sizeof(float) * (size_t)h->nnz, hipMemcpyDeviceToDevice, s));
    } else {
        h->d_v = d_val;     // not copied, not owned (may be the array as before, changed in place)
    }
    return refresh_forms(h, s);
}

int sextans_update_values(sextans_handle_t h, const float *val) {
    if (!h) return SEXTANS_ERR_INVALID;
    if (!h->d_rp) return SEXTANS_ERR_STATE;
    if (h->nnz == 0) return SEXTANS_OK;
    if (!val) return SEXTANS_ERR_INVALID;
    SX_HIP(hipSetDevice(h->device));
    if (!h->owns_matrix()) {   // a caller-provided device matrix: the uploaded values live in an array of the engine's (until the next update)
        if (!h->mat.d_v_upd) SX_HIP(h->mat.d_v_upd.alloc((size_t)h->nnz));
        h->d_v = h->mat.d_v_upd;
    }
    SX_HIP(hipDeviceSynchronize());   // nothing enqueued earlier may still read the values (synchronous, like sextans_set_matrix_csr)
    SX_HIP(hipMemcpy((void *)h->d_v, val, sizeof(float) * (size_t)h->nnz, hipMemcpyHostToDevice));
    if (int rc = refresh_forms(h, nullptr)) return rc;
    SX_HIP(hipStreamSynchronize(nullptr));
    return SEXTANS_OK;
}

}  // extern "C"
