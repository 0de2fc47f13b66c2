// pattern_launch.h -- the host side of the pattern passes (pattern_pass.h), shared by engine_attention.hip, engine_attention_edge.hip,
// engine_gat.hip, engine_gatv2.hip, engine_reduce.hip, engine_multi.hip, engine_softagg.hip, engine_edge.hip, engine_gated.hip, engine_edge_softagg.hip, engine_vector_attention.hip, engine_edge_op.hip and (through edge_multi_launch.h, the
// launcher that engine_edge_multi.hip and its per-op sources engine_edge_multi_*.hip share) the edge multi-aggregation, and included by nothing else: the launch of a pass, the width table, the
// argument checks, the degenerate-call fill, the backward's tables and the dropout variant.  What a family keeps: its Args, its entry
// points and the entries in flight per slot (U) of each of its passes.
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
inline bool bad_slope(float s) { return !(s >= 0.0f) || std::isinf(s); }
template <class... Ptr>
bool misaligned(const Ptr *...p) { return ((reinterpret_cast<uintptr_t>(p) | ... | 0) & 15) != 0; }   // some pointer is not 16-byte aligned (NULL is)

// Float goes through attention_fill (engine_state.h, defined in engine_attention.hip) so that the library holds one copy of that kernel.
template <class T>
void fill(T *out, int64_t rows, int cols, int64_t ld, T value, hipStream_t s) {
    if (!out || rows <= 0 || cols <= 0) return;
    hipLaunchKernelGGL(sx::pattern_fill<T>, dim3((unsigned)((rows * cols + 255) / 256)), dim3(256), 0, s, (long long)rows, cols, (long long)ld, value, out);
}

// what a backward with a column pass walks: the softmax tables of h, A^T behind the companion h->tr, and the companion's tables
inline int ensure_backward_tables(sextans_engine *h, hipStream_t s) {
    if (int rc = ensure_softmax_tables(h, s)) return rc;
    if (int rc = ensure_transpose(h, s)) return rc;
    return ensure_softmax_tables(h->tr, s);   // A^T's rows: the tables of the column pass
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
// last_kernel = base [+dropout] [+long_rows]
inline void name_pass(sextans_engine *h, const char *base, bool dropout, bool long_rows) {
    h->last_kernel_buf = std::string(base) + (dropout ? "+dropout" : "") + (long_rows ? "+long_rows" : "");
    h->last_kernel = h->last_kernel_buf.c_str();
}

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
