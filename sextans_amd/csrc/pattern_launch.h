// pattern_launch.h -- the host side of the pattern passes (pattern_pass.h): included by the engine_*.hip of every pattern-pass family
// and by nothing else.  The argument checks, the degenerate-call fill, the dropout variant, the frame of an entry point (PatternCall),
// the width table and the launch of a pass.  What a family keeps: its Args, the entries in flight per slot (U) of each of its passes,
// its tile cap, and its entry points -- their own argument checks, the fills of a degenerate call, and what each pass launches.
#pragma once
#include <cmath>
#include <string>

#include "dropout_hash.h"
#include "engine_state.h"
#include "pattern_pass.h"

namespace sx {

// rows x cols elements at leading dimension ld <- value (the degenerate calls: no entries, no rows)
template <class T>
__global__ __launch_bounds__(256) void pattern_fill(long long rows, int cols, long long ld, T value, T *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * cols) return;
    out[(i / cols) * ld + i % cols] = value;
}

}  // namespace sx

namespace sxe {

// --- argument checks -----------------------------------------------------------------------------------------------------------------
constexpr int kMaxTiles = 65535;   // the long-row kernel's grid has one y per column tile
inline bool bad_dim(int d) { return d < 8 || d > 128 || (d % 8) != 0; }                              // a head dimension
inline bool bad_n(int N) { return N < 8 || (N % 8) != 0 || (N + 127) / 128 > kMaxTiles; }            // the columns of a tiled family
inline bool bad_ld(int64_t ld, int64_t need) { return ld < need || (ld % 4) != 0; }
inline bool bad_ld_of(const void *p, int64_t ld, int64_t need) { return p && bad_ld(ld, need); }    // an optional operand: its leading dimension counts when it is given
inline bool too_many_tiles(int N, int max_tile) { return (N + max_tile - 1) / max_tile > kMaxTiles; }   // a family that caps its tile below 128
inline int64_t chunks_of(int64_t M) { return (M + 255) / 256; }                                      // the chunks of column_sum_two_level (engine_state.h)
inline bool bad_slope(float s) { return !(s >= 0.0f) || std::isinf(s); }
template <class... Ptr>
bool misaligned(const Ptr *...p) { return ((reinterpret_cast<uintptr_t>(p) | ... | 0) & 15) != 0; }   // some pointer is not 16-byte aligned (NULL is)

// Float goes through attention_fill (engine_state.h, defined in engine_attention.hip) so that the library holds one copy of that kernel.
template <class T>
void fill(T *out, int64_t rows, int cols, int64_t ld, T value, hipStream_t s) {
    if (!out || rows <= 0 || cols <= 0) return;
    hipLaunchKernelGGL(sx::pattern_fill<T>, dim3((unsigned)((rows * cols + 255) / 256)), dim3(256), 0, s, (long long)rows, cols, (long long)ld, value, out);
}

// --- dropout -------------------------------------------------------------------------------------------------------------------------
// drop == NULL or p == 0: the plain kernels, the plain bits
enum class Dropout { kInvalid, kPlain, kActive };
inline Dropout dropout_mode(const sextans_dropout *drop) {
    if (!drop) return Dropout::kPlain;
    if (sx::dropout_bad(drop->p, drop->d_step)) return Dropout::kInvalid;
    return drop->p == 0.0f ? Dropout::kPlain : Dropout::kActive;
}
// f(args) once: the plain args, or (drop set: dropout is active) the DropArgsT built from them
template <class DropArgsT, class Args, class F>
void with_dropout(const Args &a, const sextans_dropout *drop, F &&f) {
    if (!drop) return f(a);
    DropArgsT ad{};
    static_cast<Args &>(ad) = a;
    ad.drop = sx::dropout_args(drop->p, drop->seed, drop->d_step);
    f(ad);
}

// --- the frame of an entry point -----------------------------------------------------------------------------------------------------
// What every entry point does between its own argument checks and its return, in the order of its calls:
//     PatternCall call{h};
//     if (int rc = call.open(<a required operand is NULL>, stream)) return rc;
//     if (call.degenerate()) { <fill the outputs on call.s>; return call.done(); }
//     if (int rc = call.tables(<a column pass runs>)) return rc;
//     <Args>;  call.cols(f) and / or call.rows(f), f(engine, perm) launching the family's pass;
//     return call.close("name", dropout);
// Nothing before open's STATE return touches a non-trivial member of *h (the ABI tests hand in a zeroed buffer).
struct PatternCall {
    sextans_engine *h;
    hipStream_t s = nullptr;
    bool long_rows = false;   // some pass so far walked an engine with rows beyond kSoftmaxChunk

    // STATE without a matrix; INVALID for more entries than an int indexes and for a missing operand when there are entries; the device
    int open(bool operand_missing, void *stream) {
        if (!h->d_rp) return SEXTANS_ERR_STATE;
        if (h->nnz > INT32_MAX || (h->nnz > 0 && operand_missing)) return SEXTANS_ERR_INVALID;
        SX_HIP(hipSetDevice(h->device));
        s = (hipStream_t)stream;
        return SEXTANS_OK;
    }
    // no rows or no entries: the family fills its outputs, then done() -- last_kernel stays what it was
    bool degenerate() const { return h->M == 0 || h->nnz == 0; }
    int done() const {
        SX_HIP(hipGetLastError());
        return SEXTANS_OK;
    }
    // the softmax tables of h; cols: also A^T behind the companion h->tr and the companion's tables, what a column pass walks
    int tables(bool cols) {
        if (int rc = ensure_softmax_tables(h, s)) return rc;
        if (!cols) return SEXTANS_OK;
        if (int rc = ensure_transpose(h, s)) return rc;
        return ensure_softmax_tables(h->tr, s);
    }
    // f(e, perm): e the engine whose CSR arrays and tables the pass walks, perm NULL over A, the transpose's permutation over A^T
    template <class F>
    void walk(const sextans_engine *e, const int *perm, F &&f) {
        f(e, perm);
        long_rows |= e->softmax.nchunks > 0;
    }
    template <class F>
    void rows(F &&f) { walk(h, nullptr, f); }
    template <class F>
    void cols(F &&f) { walk(h->tr, h->at.d_tperm, f); }
    // last_kernel = name [+dropout] [+long_rows], once every launch went through
    int close(const char *name, bool dropout = false) {
        SX_HIP(hipGetLastError());
        h->last_kernel_buf = std::string(name) + (dropout ? "+dropout" : "") + (long_rows ? "+long_rows" : "");
        h->last_kernel = h->last_kernel_buf.c_str();
        return SEXTANS_OK;
    }
};

// --- launch --------------------------------------------------------------------------------------------------------------------------
// The slot widths: T lanes hold P 16-byte pieces each, 4 T P floats.
template <int T_, int P_>
struct Width {
    static constexpr int T = T_, P = P_;
    static constexpr bool k128 = 4 * T_ * P_ == 128;   // the widest one: the families halve U there
};
// f(Width<T, P>{}) for the smallest of 8 / 16 / 32 / 64 / 128 floats that holds w
template <class F>
void for_width(int w, F &&f) {
    if (w <= 8) f(Width<2, 1>{});
    else if (w <= 16) f(Width<4, 1>{});
    else if (w <= 32) f(Width<8, 1>{});
    else if (w <= 64) f(Width<8, 2>{});
    else f(Width<8, 4>{});
}
// the tiled families (reduce, edge): N in column tiles of the width, which play the heads' part
template <class W, class Args>
Args tiled(Args a) {
    a.tile = 4 * W::T * W::P;
    a.H = (a.N + a.tile - 1) / a.tile;
    return a;
}

// One pass over e's rows: e is the engine whose CSR arrays and softmax tables the pass walks (the column pass: the companion).
// inside: a slot group takes all heads (tiles) of its row one after the other; otherwise they sit in the grid.
template <class Pass>
void launch_pattern(const sextans_engine *e, const typename Pass::Args &a, const int *perm, bool inside, hipStream_t s) {
    const long long nw = (long long)e->softmax.d_sm_wrow.size() - 1;
    hipLaunchKernelGGL((sx::pattern_rows<Pass>), dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, s, a, e->d_rp, e->d_ci, perm, e->softmax.d_sm_wrow, nw,
                       inside ? 1 : 0);
    if (e->softmax.nchunks > 0)
        hipLaunchKernelGGL((sx::pattern_long<Pass>), dim3((unsigned)e->softmax.nchunks, inside ? 1u : (unsigned)a.H), dim3(256), 0, s, a, e->d_rp, e->d_ci,
                           perm, e->softmax.d_sm_tab, inside ? 1 : 0);
}

}  // namespace sxe
