"""ctypes mirror of include/sextans_amd.h -- the host-side call surface of the engine.

Every C entry point is declared once: a line of _PROTOTYPES where the Python side marshals, @_entry(<C types>) on the def line of an
Engine method that only forwards.  To add one: the prototype in the header, then one of the two; tests/test_abi_header.py holds the
table to the header, and the name is optional for older builds by derivation (_OPTIONAL_SYMBOLS).

Function names follow the reference's host library (src/sparse_helper.h, src/sextans-host.cpp) so
tests read like the reference's own harness:

    read_suitsparse_matrix  sparse_helper.h:169      CSC_2_CSR   sparse_helper.h:475
    Engine.spmm             cpu_spmm_CSR argument meaning (sparse_helper.h:262) behind the
                            tapa::invoke(Sextans, ...) boundary (sextans-host.cpp:237-251)

All compute goes through libsextans_amd.so (HIP, gfx950).  There is no Python or CPU fallback: a
missing library raises at import of this module's `lib()`; a missing GPU raises SextansError
(SEXTANS_ERR_NO_DEVICE) at Engine creation.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libsextans_amd.so")
CLI_PATH = os.path.join(_HERE, "bin", "sextans")

FMT_CSR, FMT_CSC = 0, 1
ERR_NO_DEVICE = 10

_i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
_f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
_lib = None


class Packed(C.Structure):
    """Mirror of struct sextans_packed (include/sextans_amd.h)."""
    _fields_ = [("M", C.c_int), ("K", C.c_int), ("nnz", C.c_int64), ("lanes_per_row", C.c_int),
                ("nblk", C.c_int), ("blk_row", C.POINTER(C.c_int)), ("dict_ptr", C.POINTER(C.c_int)),
                ("dict", C.POINTER(C.c_int)), ("row_off", C.POINTER(C.c_int)),
                ("idx16", C.POINTER(C.c_uint16)), ("col32", C.POINTER(C.c_int)),
                ("val", C.POINTER(C.c_float)), ("stream_len", C.c_int64), ("max_dict", C.c_int),
                ("nnz_in_panel_blocks", C.c_int64)]


class WindowPacked(C.Structure):
    """Mirror of struct sextans_window_packed (include/sextans_amd.h)."""
    _fields_ = [("M", C.c_int), ("K", C.c_int), ("nnz", C.c_int64), ("rows_per_wave", C.c_int),
                ("window_cols", C.c_int), ("nwaves", C.c_int), ("steps", C.c_int64),
                ("padded_lower_bound", C.c_int64), ("wave_step0", C.POINTER(C.c_int)),
                ("stream", C.POINTER(C.c_uint64))]


class Edges(C.Structure):
    """Mirror of struct sextans_edges (include/sextans_amd.h)."""
    _fields_ = [("M", C.c_int32), ("K", C.c_int32), ("num_windows", C.c_int32), ("num_a_len", C.c_int32),
                ("nnz", C.c_int64), ("ptr_len", C.c_int64), ("chan_len", C.c_int64),
                ("edge_list_ptr", C.POINTER(C.c_int32)), ("channel", C.POINTER(C.c_uint64) * 8)]


class Dropout(C.Structure):
    """sextans_dropout: attention dropout of the fused attention entries.  p in [0, 1), a 64-bit seed and d_step: None, or the address of
    ONE uint64 in device memory that is added to the seed (a captured graph's caller bumps it between replays)."""
    _fields_ = [("p", C.c_float), ("seed", C.c_uint64), ("d_step", C.c_void_p)]

    def __init__(self, p=0.0, seed=0, d_step=None):
        super().__init__(p, int(seed) & 0xFFFFFFFFFFFFFFFF, d_step)


class MultiOut(C.Structure):
    """sextans_multi_out: the outputs of spmm_multi_device_rm, each a device address (None: not computed) with its own leading dimension
    -- they may be column slices of one (M, k N) buffer.  ld_arg serves both args."""
    _fields_ = [("d_sum", C.c_void_p), ("d_sumsq", C.c_void_p), ("d_max", C.c_void_p), ("d_min", C.c_void_p),
                ("ld_sum", C.c_int64), ("ld_sumsq", C.c_int64), ("ld_max", C.c_int64), ("ld_min", C.c_int64),
                ("d_argmax", C.c_void_p), ("d_argmin", C.c_void_p), ("ld_arg", C.c_int64)]


class MultiGrad(C.Structure):
    """sextans_multi_grad: the upstream gradients of spmm_multi_backward_device_rm (None: absent) and the forward's args."""
    _fields_ = [("d_gsum", C.c_void_p), ("d_gsumsq", C.c_void_p), ("d_gmax", C.c_void_p), ("d_gmin", C.c_void_p),
                ("ld_gsum", C.c_int64), ("ld_gsumsq", C.c_int64), ("ld_gmax", C.c_int64), ("ld_gmin", C.c_int64),
                ("d_argmax", C.c_void_p), ("d_argmin", C.c_void_p), ("ld_arg", C.c_int64)]


class GatedIn(C.Structure):
    """sextans_gated_in: the operands of spmm_gated_device_rm as device addresses with their leading dimensions -- xdst (M x N), xsrc and
    V (K x N), E (nnz x N in the CSR entry order; None: no edge features)."""
    _fields_ = [("d_xdst", C.c_void_p), ("d_xsrc", C.c_void_p), ("d_v", C.c_void_p), ("d_e", C.c_void_p),
                ("ld_xdst", C.c_int64), ("ld_xsrc", C.c_int64), ("ld_v", C.c_int64), ("ld_e", C.c_int64)]


class GatedGrad(C.Structure):
    """sextans_gated_grad: the gradients spmm_gated_backward_device_rm writes (None: not computed; not all four)."""
    _fields_ = [("d_dxdst", C.c_void_p), ("d_dxsrc", C.c_void_p), ("d_dv", C.c_void_p), ("d_de", C.c_void_p),
                ("ld_dxdst", C.c_int64), ("ld_dxsrc", C.c_int64), ("ld_dv", C.c_int64), ("ld_de", C.c_int64)]


class SextansError(RuntimeError):
    def __init__(self, code, where=""):
        self.code = code
        msg = lib().sextans_error_string(code).decode()
        detail = lib().sextans_last_error().decode()
        super().__init__(f"{where}: [{code}] {msg}" + (f" ({detail})" if detail else ""))


DTYPE_F32, DTYPE_BF16 = 0, 1   # SEXTANS_DTYPE_*: the type of C_in / C_out on the bf16 entry points
REDUCE_MAX, REDUCE_MIN = 1, 2  # SEXTANS_REDUCE_*: the op of spmm_reduce_device_rm
EDGE_MUL, EDGE_ADD, EDGE_ADD_RELU, EDGE_COPY = 1, 2, 3, 4  # SEXTANS_EDGE_*: the op of spmm_edge_device_rm
GATE_SUM, GATE_NORM = 1, 2  # SEXTANS_GATE_*: the mode of spmm_gated_device_rm
VATT_NODE, VATT_ADD, VATT_EDGE = 1, 2, 3  # SEXTANS_VATT_*: the message of vector_attention_device_rm
EDGEOP_ADD, EDGEOP_SUB, EDGEOP_MUL, EDGEOP_DST, EDGEOP_SRC = 1, 2, 3, 4, 5  # SEXTANS_EDGEOP_*: the op of edge_op_device_rm
SCORE_SOFTMAX, SCORE_WEIGHT = 1, 2  # SEXTANS_SCORE_*: the mode of score_attention_device


# ---- the binding: one declaration per C entry point.  _PROTOTYPES maps the C name to (restype, argtypes); lib() applies it in one loop and
# tests/test_abi_header.py compares it with include/sextans_amd.h.  A function with marshalling of its own is declared in the table below;
# an Engine method that only forwards its arguments is declared by @_entry on its def line, which adds the table entry and builds the body.
i, l, f, p = C.c_int, C.c_int64, C.c_float, C.c_void_p
ref = C.POINTER    # ref(T): a struct parameter, passed C.byref(x), or None as a null pointer
_str, _dbl, _u64 = C.c_char_p, C.c_double, C.c_uint64
_ip, _lp, _dp, _pp = C.POINTER(i), C.POINTER(l), C.POINTER(_dbl), C.POINTER(p)
_ipp, _fpp, _u16pp = C.POINTER(_ip), C.POINTER(C.POINTER(f)), C.POINTER(C.POINTER(C.c_uint16))
_u16p = np.ctypeslib.ndpointer(dtype=np.uint16, flags="C_CONTIGUOUS")

_PROTOTYPES = {
    "sextans_error_string": (_str, [i]),
    "sextans_last_error": (_str, []),
    # host sparse library
    "sextans_mtx_read": (i, [_str, i, _ip, _ip, _ip, _ipp, _ipp, _fpp]),
    "sextans_mtx_read_cached": (i, [_str, _str, i, _ip, _ip, _ip, _ipp, _ipp, _fpp, _ip]),
    "sextans_mtx_write": (i, [_str, i, i, _i32p, _i32p, _f32p]),
    "sextans_matrix_save": (i, [_str, i, i, i, i, _i32p, _i32p, _f32p]),
    "sextans_matrix_load": (i, [_str, _ip, _ip, _ip, _ip, _ipp, _ipp, _fpp]),
    "sextans_host_free": (None, [p]),
    "sextans_csc_to_csr": (i, [i, i, i, _i32p, _i32p, _f32p, _i32p, _i32p, _f32p]),
    "sextans_init_dense_B": (None, [i, i, _f32p]),
    "sextans_init_dense_C": (None, [i, i, _f32p]),
    "sextans_round_up_n": (i, [i]),
    "sextans_verify": (i, [i, i, _f32p, _f32p, C.POINTER(f)]),
    "sextans_gflops": (_dbl, [i, i, l, _dbl]),
    "sextans_selfcheck_golden": (i, [i, i, i, f, _i32p, _i32p, _f32p, _f32p, f, _f32p]),
    "sextans_spmm_csr": (i, [i, i, i, i, f, _i32p, _i32p, _f32p, _f32p, f, _f32p]),
    "sextans_pack_csr": (i, [i, i, _i32p, _i32p, _f32p, i, i, C.POINTER(Packed)]),
    "sextans_packed_free": (None, [C.POINTER(Packed)]),
    "sextans_unpack_csr": (i, [C.POINTER(Packed), _i32p, _i32p, _f32p]),
    "sextans_window_pack_csr": (i, [i, i, _i32p, _i32p, _f32p, i, i, C.POINTER(WindowPacked)]),
    "sextans_window_packed_free": (None, [C.POINTER(WindowPacked)]),
    "sextans_partition_rows_by_nnz": (i, [i, _i32p, i, _i32p]),
    "sextans_dropout_keep_host": (i, [l, l, i, f, _u64, _u64, p]),
    # the accelerator's own buffer formats
    "sextans_edges_pack_csc": (i, [i, i, i, _i32p, _i32p, _f32p, C.POINTER(Edges)]),
    "sextans_edges_free": (None, [C.POINTER(Edges)]),
    "sextans_edges_decode_csr": (i, [_i32p, _pp, i, i, i, _lp, _ipp, _ipp, _fpp]),
    "sextans_edges_save": (i, [_str, C.POINTER(Edges)]),
    "sextans_edges_load": (i, [_str, C.POINTER(Edges)]),
    "sextans_chan_b_colsize": (l, [i, i]),
    "sextans_chan_b_len": (l, [i, i, i]),
    "sextans_chan_c_colsize": (l, [i]),
    "sextans_chan_c_len": (l, [i, i]),
    "sextans_chan_pack_b": (i, [i, i, i, _f32p, _pp]),
    "sextans_chan_unpack_b": (i, [i, i, i, _pp, _f32p]),
    "sextans_chan_pack_c": (i, [i, i, _f32p, _pp]),
    "sextans_chan_unpack_c": (i, [i, i, _pp, _f32p]),
    # the engine: the entry points whose Engine method marshals (the forwarding ones are declared by @_entry)
    "sextans_device_count": (i, [_ip]),
    "sextans_create": (i, [_pp, i]),
    "sextans_destroy": (i, [p]),
    "sextans_set_option": (i, [p, _str, l]),
    "sextans_get_option": (i, [p, _str, _lp]),
    "sextans_get_stat": (i, [p, _str, _dp]),
    "sextans_align_row": (i, [p, i, i, _ip]),
    "sextans_reassociated_rows": (i, [p, _i32p, i, _ip]),
    "sextans_export_plan": (i, [p, i, C.POINTER(Packed)]),
    "sextans_export_row_order": (i, [p, _i32p, _ip]),
    "sextans_set_matrix_csr": (i, [p, i, i, l, _i32p, _i32p, _f32p]),
    "sextans_set_matrix_csr_device": (i, [p, i, i, l, p, p, p]),
    "sextans_set_matrix_edges": (i, [p, _i32p, _pp, i, i, i, i]),
    "sextans_set_matrix_bell": (i, [p, i, i, i, _i32p, _u16p]),
    "sextans_update_values": (i, [p, p]),
    "sextans_prepare": (i, [p, i, i, p]),
    "sextans_prepare_rm_bf16": (i, [p, i, i, i, p]),
    "sextans_spmm_host": (i, [p, i, f, _f32p, f, _f32p, i, _dp]),
    "sextans_invoke": (i, [p, p, _pp, _pp, i, _pp, _pp, i, i, i, i, i, i, i, _dp]),
    "sextans_spmm_device_rows": (i, [p, i, f, p, l, f, p, l, p, l, i, i, i, p]),
    "sextans_profile_read": (i, [p, _dp, _lp, _dp]),
    "sextans_profile_read_post": (i, [p, _dp, _lp]),
    "sextans_phase_timing_read": (i, [p, _lp]),
    "sextans_last_kernel": (_str, [p]),
    # several GPUs
    "sextans_dist_bind_library": (i, [_str]),
    "sextans_dist_unique_id": (i, [_str]),
    "sextans_dist_comm_init": (i, [_pp, i, i, i, _str]),
    "sextans_dist_comm_destroy": (i, [p]),
    "sextans_dist_prepare": (i, [p, p, i, i, _i32p, i, i, i, p]),
    "sextans_dist_spmm": (i, [p, p, i, i, _i32p, i, f, p, l, f, p, l, p, l, i, p]),
    "sextans_dist_spmm_rm": (i, [p, p, i, i, _i32p, i, f, p, l, f, p, l, p, l, p]),
    "sextans_dist_spmm_bell": (i, [p, p, i, i, _i32p, i, f, p, l, f, p, l, p, l, p]),
    # synthetic inputs and device memory
    "sextans_gen_csr_host": (i, [i, i, _dbl, i, _u64, i, i, _ipp, _ipp, _fpp, _lp]),
    "sextans_gen_csr_device": (i, [i, i, i, _dbl, i, _u64, i, i, _pp, _pp, _pp, _lp]),
    "sextans_gen_stencil2d_host": (i, [i, i, i, i, _u64, i, i, _ipp, _ipp, _fpp, _lp]),
    "sextans_gen_stencil2d_device": (i, [i, i, i, i, i, _u64, i, i, _pp, _pp, _pp, _lp]),
    "sextans_gen_kkt_host": (i, [i, i, _u64, i, i, _ipp, _ipp, _fpp, _lp]),
    "sextans_gen_kkt_device": (i, [i, i, i, _u64, i, i, _pp, _pp, _pp, _lp]),
    "sextans_gen_fem3d_host": (i, [i, i, i, i, _u64, i, i, _ipp, _ipp, _fpp, _lp]),
    "sextans_gen_fem3d_device": (i, [i, i, i, i, i, _u64, i, i, _pp, _pp, _pp, _lp]),
    "sextans_gen_powerlaw_host": (i, [i, i, i, i, i, _u64, i, i, _ipp, _ipp, _fpp, _lp]),
    "sextans_gen_powerlaw_device": (i, [i, i, i, i, i, i, _u64, i, i, _pp, _pp, _pp, _lp]),
    "sextans_gen_kron_host": (i, [i, i, i, _i32p, _i32p, i, _u64, i, i, _ipp, _ipp, _fpp, _lp, _ip]),
    "sextans_gen_kron_device": (i, [i, i, i, i, _i32p, _i32p, i, _u64, i, i, _pp, _pp, _pp, _lp, _ip]),
    "sextans_gen_bell_host": (i, [i, i, i, _u64, _ipp, _u16pp]),
    "sextans_gen_bell_device": (i, [i, i, i, i, _u64, _pp, _pp]),
    "sextans_gen_bell_banded_host": (i, [i, i, i, _u64, _ipp, _u16pp]),
    "sextans_gen_bell_banded_device": (i, [i, i, i, i, _u64, _pp, _pp]),
    "sextans_gen_uniform_host": (i, [_f32p, l, _u64]),
    "sextans_gen_uniform_device": (i, [i, p, l, _u64, p]),
    "sextans_gen_uniform_bf16_host": (i, [_u16p, l, _u64]),
    "sextans_gen_uniform_bf16_device": (i, [i, p, l, _u64, p]),
    "sextans_device_alloc": (i, [i, C.c_size_t, _pp]),
    "sextans_device_copy": (i, [i, p, p, C.c_size_t, i]),
    "sextans_device_free": (i, [i, p]),
    "sextans_csr_transpose_device": (i, [i, i, i, l, p, p, p, _pp, _pp, _pp, p]),
    "sextans_csr_permute_symmetric_device": (i, [i, i, l, p, p, p, p, _pp, _pp, _pp]),
    "sextans_csr_slice_rows_device": (i, [i, i, i, p, _pp, _lp, _lp]),
}

# The entry points that existed by round 4: the only ones every build must export.  The set never grows; every later name is optional
# (_OPTIONAL_SYMBOLS, at the end of this module), so that the library of an earlier round still loads for a same-box A/B (tools/nasa_ab.py).
_ROUND4_SYMBOLS = frozenset("sextans_" + name for name in """
    align_row chan_b_colsize chan_b_len chan_c_colsize chan_c_len chan_pack_b chan_pack_c chan_unpack_b chan_unpack_c create
    csc_to_csr destroy device_count device_free dist_comm_destroy dist_comm_init dist_spmm dist_unique_id edges_decode_csr edges_free
    edges_load edges_pack_csc edges_save error_string export_plan gen_bell_banded_device gen_bell_banded_host gen_bell_device
    gen_bell_host gen_csr_device gen_csr_host gen_fem3d_device gen_fem3d_host gen_kkt_device gen_kkt_host gen_powerlaw_device
    gen_powerlaw_host gen_stencil2d_device gen_stencil2d_host gen_uniform_bf16_device gen_uniform_bf16_host gen_uniform_device
    gen_uniform_host get_option get_stat gflops host_free init_dense_B init_dense_C invoke last_error last_kernel mtx_read pack_csr
    packed_free partition_rows_by_nnz phase_timing_read profile_read profile_reset reassociated_rows round_up_n selfcheck_golden
    set_matrix_bell set_matrix_bell_device set_matrix_csr set_matrix_csr_device set_matrix_edges set_option spmm_bell_device spmm_csr
    spmm_device spmm_device2 spmm_device_rows spmm_host unpack_csr verify window_pack_csr window_packed_free""".split())


def _bind(L):
    """Declare every prototype of _PROTOTYPES on the library L.  An entry point that L lacks is skipped when it is optional -- calling it
    later fails with ctypes' own AttributeError -- and fails the load when it is one of _ROUND4_SYMBOLS: a typo or a broken build (without
    its prototype ctypes would truncate 64-bit arguments to int)."""
    for name, (restype, argtypes) in _PROTOTYPES.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            if name in _ROUND4_SYMBOLS:
                raise
            continue
        fn.restype, fn.argtypes = restype, argtypes
    return L


def lib():
    """Load libsextans_amd.so once.  torch (if importable) is imported first so that this library
    binds to the same libamdhip64.so.7 instance torch uses (one HIP runtime per process)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build the HIP engine with `python -m sextans_amd.build` "
            "(there is no CPU fallback)")
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    _lib = _bind(C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL))
    return _lib


_FORWARD = """def {name}(self, {params}):
    _check(lib().sextans_{name}(self._h, {args}), "{name}")
"""
_COUNT = """def {name}(self, {params}):
    n = lib().sextans_{name}(self._h, {args})
    if n < 0:
        _check(int(-n), "{name}")
    return int(n)
"""


def _entry(*kinds, result=i):
    """Declare the Engine method under it as the C entry point sextans_<its name>(handle, <kinds>[, stream]): kinds are the C types of
    its parameters between self and a trailing `stream`, one each (checked here, at import).  The prototype goes into _PROTOTYPES; the
    method keeps its def line and docstring and gets its body from a template compiled once, as collections.namedtuple does: the plain
    forwarding call, a ref(T) parameter passed by address; with result=l, a count whose negative value is the error code."""
    def declare(fn):
        names = fn.__code__.co_varnames[1:fn.__code__.co_argcount]
        streamed = names[-1:] == ("stream",)
        if len(kinds) != len(names) - streamed:
            raise TypeError(f"{fn.__name__}: {len(kinds)} C types for {len(names) - streamed} parameters")
        _PROTOTYPES["sextans_" + fn.__name__] = (result, [p, *kinds] + [p] * streamed)
        args = [f"C.byref({n}) if {n} is not None else None" if issubclass(k, C._Pointer) else n for n, k in zip(names, kinds)]
        scope = {}
        exec((_FORWARD if result is i else _COUNT).format(name=fn.__name__, params=", ".join(names),
                                                         args=", ".join(args + ["stream"] * streamed)), globals(), scope)
        new = scope[fn.__name__]
        new.__defaults__, new.__doc__, new.__qualname__ = fn.__defaults__, fn.__doc__, fn.__qualname__
        return new
    return declare


def _frame(method):
    """The kinds of an Engine method declared above, for a twin that takes the same frame."""
    return _PROTOTYPES["sextans_" + method][1][1:-1]


def _check(rc, where):
    if rc != 0:
        raise SextansError(rc, where)


def _buf(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a if a.size else np.zeros(1, dtype)


def _take(ptr, n, dtype):
    if n == 0:
        return np.zeros(0, dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True)


# ------------------------------------------------------------------ L2: host sparse library

def read_suitsparse_matrix(path, fmt=FMT_CSR, cache=None):
    """-> (ptr, idx, val, M, K, nnz); raises SextansError where the reference would exit(1).
    cache: None = parse the text; True = go through the binary container next to the file
    (path + ".csr.sxbin" / ".csc.sxbin"); a string = that container path."""
    L = lib()
    M, K, nnz = C.c_int(), C.c_int(), C.c_int()
    p, i, v = C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.POINTER(C.c_float)()
    if cache is None:
        _check(L.sextans_mtx_read(os.fsencode(path), fmt, M, K, nnz, p, i, v), f"mtx_read({path})")
    else:
        hit = C.c_int()
        cpath = None if cache is True else os.fsencode(cache)
        _check(L.sextans_mtx_read_cached(os.fsencode(path), cpath, fmt, M, K, nnz, p, i, v, C.byref(hit)),
               f"mtx_read_cached({path})")
        read_suitsparse_matrix.last_cache_hit = bool(hit.value)
    n_ptr = (M.value if fmt == FMT_CSR else K.value) + 1
    out = (_take(p, n_ptr, np.int32), _take(i, nnz.value, np.int32),
           _take(v, nnz.value, np.float32), M.value, K.value, nnz.value)
    for q in (p, i, v):
        L.sextans_host_free(q)
    return out


def matrix_save(path, fmt, M, K, ptr, idx, val):
    _check(lib().sextans_matrix_save(os.fsencode(path), fmt, M, K, int(len(idx)), _buf(ptr, np.int32),
                                     _buf(idx, np.int32), _buf(val, np.float32)), f"matrix_save({path})")


def matrix_load(path):
    """-> (fmt, ptr, idx, val, M, K, nnz)"""
    L = lib()
    fmt, M, K, nnz = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    p, i, v = C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.POINTER(C.c_float)()
    _check(L.sextans_matrix_load(os.fsencode(path), fmt, M, K, nnz, p, i, v), f"matrix_load({path})")
    n_ptr = (M.value if fmt.value == FMT_CSR else K.value) + 1
    out = (fmt.value, _take(p, n_ptr, np.int32), _take(i, nnz.value, np.int32), _take(v, nnz.value, np.float32),
           M.value, K.value, nnz.value)
    for q in (p, i, v):
        L.sextans_host_free(q)
    return out


def CSC_2_CSR(M, K, NNZ, csc_col_ptr, csc_row_idx, csc_val):
    rp = np.zeros(M + 1, np.int32)
    ci = np.zeros(max(NNZ, 1), np.int32)
    cv = np.zeros(max(NNZ, 1), np.float32)
    _check(lib().sextans_csc_to_csr(M, K, NNZ, _buf(csc_col_ptr, np.int32),
                                    _buf(csc_row_idx, np.int32), _buf(csc_val, np.float32),
                                    rp, ci, cv), "csc_to_csr")
    return rp, ci[:NNZ].copy(), cv[:NNZ].copy()


def pack_csr(M, K, row_ptr, col_idx, val, lanes_per_row=4, min_reuse_x100=400):
    """Build the packed row-bucketed form (host); returns a dict of numpy arrays + scalars."""
    L = lib()
    P = Packed()
    _check(L.sextans_pack_csr(M, K, _buf(row_ptr, np.int32), _buf(col_idx, np.int32), _buf(val, np.float32),
                              lanes_per_row, min_reuse_x100, C.byref(P)), "pack_csr")
    try:
        nb, sl = P.nblk, P.stream_len
        out = dict(M=P.M, K=P.K, nnz=P.nnz, lanes_per_row=P.lanes_per_row, nblk=nb, stream_len=sl,
                   max_dict=P.max_dict, nnz_in_panel_blocks=P.nnz_in_panel_blocks,
                   blk_row=_take(P.blk_row, nb + 1, np.int32), dict_ptr=_take(P.dict_ptr, nb + 1, np.int32),
                   row_off=_take(P.row_off, M + 1, np.int32), idx16=_take(P.idx16, sl, np.uint16),
                   col32=_take(P.col32, sl, np.int32), val=_take(P.val, sl, np.float32))
        out["dict"] = _take(P.dict, int(out["dict_ptr"][-1]), np.int32)
        # decode through the C decoder as well
        ci = np.zeros(max(int(P.nnz), 1), np.int32)
        va = np.zeros(max(int(P.nnz), 1), np.float32)
        _check(L.sextans_unpack_csr(C.byref(P), _buf(row_ptr, np.int32), ci, va), "unpack_csr")
        out["decoded_col_idx"], out["decoded_val"] = ci[:P.nnz], va[:P.nnz]
        return out
    finally:
        L.sextans_packed_free(C.byref(P))


def window_pack_csr(M, K, row_ptr, col_idx, val, rows_per_wave=319, window_cols=65536):
    """Build the K-windowed stream of the accumulator-resident kernel (host); returns a dict:
    wave_step0[nwaves+1], val[steps*32] (float32), row[steps*32] (local row; == rows_per_wave for padding),
    col[steps*32]."""
    L = lib()
    P = WindowPacked()
    _check(L.sextans_window_pack_csr(M, K, _buf(row_ptr, np.int32), _buf(col_idx, np.int32),
                                     _buf(val, np.float32), rows_per_wave, window_cols, C.byref(P)),
           "window_pack_csr")
    try:
        n = int(P.steps) * 32
        words = _take(P.stream, n, np.uint64)
        hi = (words >> np.uint64(32)).astype(np.uint32)
        return dict(M=P.M, K=P.K, nnz=P.nnz, rows_per_wave=P.rows_per_wave, window_cols=P.window_cols,
                    nwaves=P.nwaves, steps=int(P.steps), padded_lower_bound=int(P.padded_lower_bound),
                    wave_step0=_take(P.wave_step0, P.nwaves + 1, np.int32),
                    val=(words & np.uint64(0xffffffff)).astype(np.uint32).view(np.float32),
                    row=(hi >> np.uint32(23)).astype(np.int32), col=(hi & np.uint32(0x7fffff)).astype(np.int32))
    finally:
        L.sextans_window_packed_free(C.byref(P))


# ---- the accelerator's own buffer formats ----

def _rows(a2d):
    """(void *)[n] over the rows of a C-contiguous 2-D array (one pointer per channel)."""
    n = a2d.shape[0]
    arr = (C.c_void_p * n)()
    for i in range(n):
        arr[i] = a2d[i].ctypes.data
    return arr


def _edges_to_dict(E):
    ch = np.stack([_take(E.channel[c], E.chan_len, np.uint64) if E.chan_len else np.zeros(0, np.uint64)
                   for c in range(8)])
    return dict(M=E.M, K=E.K, num_windows=E.num_windows, num_a_len=E.num_a_len, nnz=E.nnz,
                edge_list_ptr=_take(E.edge_list_ptr, E.ptr_len, np.int32), channels=ch)


def edges_pack_csc(M, K, col_ptr, row_idx, val):
    """generate_edge_list_for_all_PEs + edge_list_64bit + the edge_list_ptr padding
    (sextans-host.cpp:114-146): -> dict(edge_list_ptr[ptr_len], channels[8, chan_len] uint64, ...)."""
    L = lib()
    E = Edges()
    _check(L.sextans_edges_pack_csc(M, K, int(len(row_idx)), _buf(col_ptr, np.int32), _buf(row_idx, np.int32),
                                    _buf(val, np.float32), C.byref(E)), "edges_pack_csc")
    try:
        return _edges_to_dict(E)
    finally:
        L.sextans_edges_free(C.byref(E))


def edges_decode_csr(edge_list_ptr, channels, num_windows, M, K):
    """-> (row_ptr, col_idx, val): each row's entries in stream order."""
    L = lib()
    ch = np.ascontiguousarray(channels, np.uint64)
    if ch.shape[1] == 0:
        ch = np.zeros((8, 1), np.uint64)
    nnz = C.c_int64()
    p, i, v = C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.POINTER(C.c_float)()
    _check(L.sextans_edges_decode_csr(_buf(edge_list_ptr, np.int32), _rows(ch), num_windows, M, K, C.byref(nnz),
                                      p, i, v), "edges_decode_csr")
    out = (_take(p, M + 1, np.int32), _take(i, nnz.value, np.int32), _take(v, nnz.value, np.float32))
    for q in (p, i, v):
        L.sextans_host_free(q)
    return out


def edges_save(path, e):
    """Write the container file from a dict as returned by edges_pack_csc."""
    L = lib()
    ch = np.ascontiguousarray(e["channels"], np.uint64)
    ptr = np.ascontiguousarray(e["edge_list_ptr"], np.int32)
    E = Edges(M=e["M"], K=e["K"], num_windows=e["num_windows"], num_a_len=e["num_a_len"], nnz=e["nnz"],
              ptr_len=ptr.size, chan_len=ch.shape[1])
    E.edge_list_ptr = ptr.ctypes.data_as(C.POINTER(C.c_int32))
    for c in range(8):
        E.channel[c] = ch[c].ctypes.data_as(C.POINTER(C.c_uint64))
    _check(L.sextans_edges_save(os.fsencode(path), C.byref(E)), f"edges_save({path})")


def edges_load(path):
    L = lib()
    E = Edges()
    _check(L.sextans_edges_load(os.fsencode(path), C.byref(E)), f"edges_load({path})")
    try:
        return _edges_to_dict(E)
    finally:
        L.sextans_edges_free(C.byref(E))


def chan_pack_b(K, N, B, num_ch_b=4):
    """mat_B_cpu (column major K x N) -> mat_B_fpga_vec[num_ch_b][len] (sextans-host.cpp:152-177)."""
    L = lib()
    ch = np.zeros((num_ch_b, L.sextans_chan_b_len(K, N, num_ch_b)), np.float32)
    _check(L.sextans_chan_pack_b(K, N, num_ch_b, _buf(B, np.float32), _rows(ch)), "chan_pack_b")
    return ch


def chan_unpack_b(K, N, channels):
    ch = np.ascontiguousarray(channels, np.float32)
    B = np.zeros(K * N, np.float32)
    _check(lib().sextans_chan_unpack_b(K, N, ch.shape[0], _rows(ch), _buf(B, np.float32)), "chan_unpack_b")
    return B


def chan_pack_c(M, N, Cm):
    """mat_C_cpu (column major M x N) -> mat_C_fpga_in[8][len] (sextans-host.cpp:179-195)."""
    L = lib()
    ch = np.zeros((8, L.sextans_chan_c_len(M, N)), np.float32)
    _check(L.sextans_chan_pack_c(M, N, _buf(Cm, np.float32), _rows(ch)), "chan_pack_c")
    return ch


def chan_unpack_c(M, N, channels):
    """mat_C_fpga_vec[8][len] -> column major M x N (the indexing of sextans-host.cpp:264-270)."""
    ch = np.ascontiguousarray(channels, np.float32)
    Cm = np.zeros(M * N, np.float32)
    out = _buf(Cm, np.float32)
    _check(lib().sextans_chan_unpack_c(M, N, _rows(ch), out), "chan_unpack_c")
    return out[:M * N]


def init_dense_B(K, N):
    B = np.empty(K * N, np.float32)
    lib().sextans_init_dense_B(K, N, _buf(B, np.float32) if B.size == 0 else B)
    return B


def init_dense_C(M, N):
    Cm = np.empty(M * N, np.float32)
    lib().sextans_init_dense_C(M, N, _buf(Cm, np.float32) if Cm.size == 0 else Cm)
    return Cm


def round_up_n(N):
    return lib().sextans_round_up_n(N)


def verify(M, N, c_cpu, c_dev):
    pct = C.c_float()
    n = lib().sextans_verify(M, N, _buf(c_cpu, np.float32), _buf(c_dev, np.float32), C.byref(pct))
    return n, pct.value


def gflops(M, N, nnz, seconds):
    return lib().sextans_gflops(M, N, nnz, seconds)


def device_count():
    n = C.c_int()
    rc = lib().sextans_device_count(C.byref(n))
    return 0 if rc else n.value


# ------------------------------------------------------------------ L1: the engine

class Engine:
    """One engine per HIP device; upload A once, launch SpMM many times."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        self.device = device
        _check(lib().sextans_create(C.byref(self._h), device), "sextans_create")
        self.M = self.K = self.nnz = 0

    def close(self):
        if self._h:
            lib().sextans_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_option(self, key, value):
        _check(lib().sextans_set_option(self._h, key.encode(), int(value)), f"set_option({key})")

    def dist_spmm(self, comm, world, rank, ranges, N, alpha, d_B, ldb, beta, d_C_in, ldc_in, d_C_out, ldc, nchunks=4,
                  stream=None):
        """Native multi-GPU SpMM (sextans_dist_spmm): this engine holds rows ranges[rank] of the matrix."""
        rr = np.ascontiguousarray(np.asarray(ranges, np.int32).reshape(-1))
        _check(lib().sextans_dist_spmm(self._h, comm, world, rank, rr, N, alpha, d_B, ldb, beta, d_C_in, ldc_in,
                                       d_C_out, ldc, nchunks, stream), "dist_spmm")

    def dist_spmm_rm(self, comm, world, rank, ranges, N, alpha, d_B, ldb, beta, d_C_in, ldc_in, d_C_out, ldc, stream=None):
        """Native multi-GPU SpMM on ROW-major operands (sextans_dist_spmm_rm): the rank's rows are written in place, the exchange is an
        in-place all-gather of contiguous row runs."""
        rr = np.ascontiguousarray(np.asarray(ranges, np.int32).reshape(-1))
        _check(lib().sextans_dist_spmm_rm(self._h, comm, world, rank, rr, N, alpha, d_B, ldb, beta, d_C_in, ldc_in, d_C_out, ldc, stream),
               "dist_spmm_rm")

    def prepare(self, N, rowmajor=False, stream=None, *, transposed=False):
        """Build everything the first SpMM call for N columns would build inside itself (sextans_prepare); transposed=True (keyword only,
        so that prepare(N, rowmajor, stream) keeps its meaning): also A^T and the plans of the transposed row-major calls
        (SEXTANS_LAYOUT_ROWMAJOR_T)."""
        _check(lib().sextans_prepare(self._h, N, 1 if rowmajor else 0, stream), "sextans_prepare")
        if transposed:
            _check(lib().sextans_prepare(self._h, N, 3, stream), "sextans_prepare(transposed)")

    def dist_prepare(self, comm, world, rank, ranges, N, nchunks=4, form=0, stream=None):
        """Collective: exchanges, plan build, tables and workspaces of the dist entry point `form` (0 sextans_dist_spmm, 1 _rm, 2 _bell)
        outside the timed call; OK on all ranks or an error on all ranks (sextans_dist_prepare)."""
        rr = np.ascontiguousarray(np.asarray(ranges, np.int32).reshape(-1))
        _check(lib().sextans_dist_prepare(self._h, comm, world, rank, rr, N, nchunks, form, stream),
               "sextans_dist_prepare")

    def export_plan(self, lanes_per_row=4):
        """The packed row-bucketed form the engine built ON THE DEVICE for the current matrix, read back in the layout of
        pack_csr (the host builder of the same format): dict of numpy arrays + scalars."""
        P = Packed()
        _check(lib().sextans_export_plan(self._h, lanes_per_row, C.byref(P)), "export_plan")
        try:
            nb, sl, M = P.nblk, P.stream_len, P.M
            out = dict(M=P.M, K=P.K, nnz=P.nnz, lanes_per_row=P.lanes_per_row, nblk=nb, stream_len=sl,
                       max_dict=P.max_dict, nnz_in_panel_blocks=P.nnz_in_panel_blocks,
                       blk_row=_take(P.blk_row, nb + 1, np.int32), dict_ptr=_take(P.dict_ptr, nb + 1, np.int32),
                       row_off=_take(P.row_off, M + 1, np.int32), idx16=_take(P.idx16, sl, np.uint16),
                       col32=_take(P.col32, sl, np.int32), val=_take(P.val, sl, np.float32))
            out["dict"] = _take(P.dict, int(out["dict_ptr"][-1]), np.int32)
            return out
        finally:
            lib().sextans_packed_free(C.byref(P))

    def export_row_order(self):
        """(order, kind): order[i] = row at position i of the clustered plan (identity when kind == 0); see include/sextans_amd.h."""
        order, kind = np.empty(max(self.M, 1), np.int32), C.c_int()
        _check(lib().sextans_export_row_order(self._h, order, C.byref(kind)), "export_row_order")
        return order[:self.M], kind.value

    def reassociated_rows(self):
        """Hub rows whose sums are formed in pieces under the current "split_rows" setting (ascending)."""
        n = C.c_int()
        _check(lib().sextans_reassociated_rows(self._h, np.zeros(1, np.int32), 0, C.byref(n)), "reassociated_rows")
        rows = np.zeros(max(n.value, 1), np.int32)
        _check(lib().sextans_reassociated_rows(self._h, rows, n.value, C.byref(n)), "reassociated_rows")
        return rows[:n.value]

    def align_row(self, N, row):
        """Largest row <= `row` where a row-range call keeps the whole-matrix kernel (sextans_align_row)."""
        out = C.c_int()
        _check(lib().sextans_align_row(self._h, N, int(row), C.byref(out)), "align_row")
        return out.value

    def get_stat(self, key):
        v = C.c_double()
        _check(lib().sextans_get_stat(self._h, key.encode(), C.byref(v)), f"get_stat({key})")
        return v.value

    def get_option(self, key):
        v = C.c_int64()
        _check(lib().sextans_get_option(self._h, key.encode(), C.byref(v)), f"get_option({key})")
        return v.value

    def set_matrix_csr(self, M, K, row_ptr, col_idx, val):
        nnz = int(np.asarray(col_idx).shape[0])
        _check(lib().sextans_set_matrix_csr(self._h, M, K, nnz, _buf(row_ptr, np.int32),
                                            _buf(col_idx, np.int32), _buf(val, np.float32)),
               "set_matrix_csr")
        self.M, self.K, self.nnz = M, K, nnz

    def set_matrix_csr_device(self, M, K, nnz, d_row_ptr, d_col_idx, d_val):
        _check(lib().sextans_set_matrix_csr_device(self._h, M, K, nnz, d_row_ptr, d_col_idx,
                                                   d_val), "set_matrix_csr_device")
        self.M, self.K, self.nnz = M, K, nnz

    def update_values(self, val):
        """New values (host array, nnz floats in the CSR entry order the matrix was set with) for the pattern that is set: every packed
        form that exists is rewritten, nothing is planned again (sextans_update_values; synchronous)."""
        v = np.ascontiguousarray(val, dtype=np.float32)
        if self.nnz and v.size != self.nnz:   # (nnz is not known here for a matrix set from edge lists)
            raise ValueError("update_values needs one value per stored entry of the matrix that is set")
        _check(lib().sextans_update_values(self._h, v.ctypes.data if v.size else None), "update_values")

    @_entry(p)
    def update_values_device(self, d_val, stream=None):
        """The same for a device array (sextans_update_values_device): it BECOMES the value array of a matrix set with
        set_matrix_csr_device (not copied; may be the pointer as before = changed in place), and is copied into the array of a matrix the
        engine owns.  Enqueued on `stream`; with default options it allocates nothing and does not synchronise (capturable)."""

    def spmm(self, N, alpha, B, beta, C_inout, rp_time=1):
        """Host buffers, C updated in place (cpu_spmm_CSR semantics).  Returns device ns for all
        rp_time repeats (what tapa::invoke returns, sextans-host.cpp:237)."""
        B = np.ascontiguousarray(B, np.float32)
        if not (isinstance(C_inout, np.ndarray) and C_inout.dtype == np.float32
                and C_inout.flags.c_contiguous):
            raise TypeError("C must be a contiguous float32 numpy array (updated in place)")
        if B.size != self.K * N or C_inout.size != self.M * N:
            raise ValueError("B must hold K*N and C must hold M*N floats")
        ns = C.c_double()
        _check(lib().sextans_spmm_host(self._h, N, alpha, _buf(B, np.float32), beta,
                                       C_inout if C_inout.size else np.zeros(1, np.float32),
                                       rp_time, C.byref(ns)), "spmm_host")
        return ns.value

    def set_matrix_edges(self, edge_list_ptr, channels, NUM_ITE, NUM_A_LEN, M, K):
        ch = np.ascontiguousarray(channels, np.uint64)
        _check(lib().sextans_set_matrix_edges(self._h, _buf(edge_list_ptr, np.int32), _rows(ch), NUM_ITE,
                                              NUM_A_LEN, M, K), "set_matrix_edges")
        self.M, self.K = M, K

    def invoke(self, edge_list_ptr, edge_list_ch, mat_B_ch, mat_C_ch_in, NUM_ITE, NUM_A_LEN, M, K, P_N,
               alpha_u, beta_u, mat_C_ch=None):
        """tapa::invoke(Sextans, ...)'s argument list (sextans-host.cpp:237-251) on numpy buffers.
        edge_list_ptr=None reuses the matrix already set.  -> (mat_C_ch[8, len], elapsed_ns)."""
        bch = np.ascontiguousarray(mat_B_ch, np.float32)
        cin = np.ascontiguousarray(mat_C_ch_in, np.float32)
        cout = np.zeros_like(cin) if mat_C_ch is None else mat_C_ch
        ns = C.c_double()
        if edge_list_ptr is None:
            ptr, ach = None, (C.c_void_p * 8)()
        else:
            ptr_arr = _buf(edge_list_ptr, np.int32)
            ach_arr = np.ascontiguousarray(edge_list_ch, np.uint64)
            ptr, ach = ptr_arr.ctypes.data, _rows(ach_arr)
        _check(lib().sextans_invoke(self._h, ptr, ach, _rows(bch), bch.shape[0], _rows(cin), _rows(cout),
                                    NUM_ITE, NUM_A_LEN, M, K, P_N, alpha_u, beta_u, C.byref(ns)), "invoke")
        self.M, self.K = M, K
        return cout, ns.value

    @_entry(i, f, p, l, f, p, p, l)
    def spmm_device(self, N, alpha, d_B, ldb, beta, d_C_in, d_C_out, ldc, stream=None):
        ...

    # ---- blocked-ELL bf16 path (BASELINE config 5)
    def set_matrix_bell(self, M, K, ell_width, block_col, block_val_bf16):
        _check(lib().sextans_set_matrix_bell(self._h, M, K, ell_width, _buf(block_col, np.int32),
                                             _buf(block_val_bf16, np.uint16)), "set_matrix_bell")

    @_entry(i, i, i, p, p)
    def set_matrix_bell_device(self, M, K, ell_width, d_block_col, d_block_val):
        ...

    @_entry(i, f, p, l, f, p, p, l)
    def spmm_bell_device(self, N, alpha, d_B_bf16, ldb, beta, d_C_in, d_C_out, ldc, stream=None):
        ...

    @_entry(i, f, p, l, f, p, l, p, l)
    def spmm_bell_device2(self, N, alpha, d_B_bf16, ldb, beta, d_C_in, ldc_in, d_C_out, ldc, stream=None):
        ...

    def dist_spmm_bell(self, comm, world, rank, ranges, N, alpha, d_B_bf16, ldb, beta, d_C_in, ldc_in, d_C_out, ldc, stream=None):
        """Blocked-ELL over several GPUs (sextans_dist_spmm_bell): this engine holds the block rows of ranges[rank]."""
        rr = np.ascontiguousarray(np.asarray(ranges, np.int32).reshape(-1))
        _check(lib().sextans_dist_spmm_bell(self._h, comm, world, rank, rr, N, alpha, d_B_bf16, ldb, beta, d_C_in, ldc_in, d_C_out, ldc, stream),
               "dist_spmm_bell")

    @_entry(i, f, p, l, f, p, l, p, l)
    def spmm_device2(self, N, alpha, d_B, ldb, beta, d_C_in, ldc_in, d_C_out, ldc_out, stream=None):
        ...

    @_entry(i, f, p, l, f, p, l, p, l)
    def spmm_device_rm(self, N, alpha, d_B, ldb, beta, d_C_in, ldc_in, d_C_out, ldc_out, stream=None):
        """ROW-major operands (B[k * ldb + n], C[m * ldc + n]): no layout pass on the LDS-panel paths (include/sextans_amd.h)."""

    @_entry(i, f, p, l, f, p, l, p, l)
    def spmm_t_device_rm(self, N, alpha, d_B, ldb, beta, d_C_in, ldc_in, d_C_out, ldc_out, stream=None):
        """C (K x N) = alpha * A^T * B + beta * C_in, B M x N, all ROW-major; A^T is built once and served by a companion engine with
        this engine's options (sextans_spmm_t_device_rm)."""

    @_entry(i, f, p, l, f, p, l, p, l, i)
    def spmm_device_rm_bf16(self, N, alpha, d_B, ldb, beta, d_C_in, ldc_in, d_C_out, ldc_out, c_dtype=DTYPE_F32, stream=None):
        """ROW-major operands with B in bf16 and C_in / C_out both fp32 (DTYPE_F32) or bf16 (DTYPE_BF16); ld in elements.  The fp32
        result has the bits of spmm_device_rm on the widened operands; native on the gather path, through fp32 copies elsewhere
        (sextans_spmm_device_rm_bf16; stats "bf16_native_calls" / "bf16_converted_calls")."""

    @_entry(*_frame("spmm_device_rm_bf16"))
    def spmm_t_device_rm_bf16(self, N, alpha, d_B, ldb, beta, d_C_in, ldc_in, d_C_out, ldc_out, c_dtype=DTYPE_F32, stream=None):
        """The same for A^T (B is M x N, C is K x N), on the companion engine of spmm_t_device_rm (sextans_spmm_t_device_rm_bf16)."""

    def prepare_rm_bf16(self, N, c_dtype, transposed=False, stream=None):
        """Everything a later bf16 call for (N, c_dtype) would build or allocate, built now (sextans_prepare_rm_bf16)."""
        _check(lib().sextans_prepare_rm_bf16(self._h, N, c_dtype, 1 if transposed else 0, stream), "prepare_rm_bf16")

    @_entry(i, f, p, l, p, l, f, p, p)
    def sddmm_device_rm(self, N, alpha, d_X, ldx, d_Y, ldy, beta, d_vals_in, d_vals_out, stream=None):
        """vals_out[e] = alpha * sum_n X[r, n] * Y[c, n] (+ beta * vals_in[e]) for every entry e = (r, c) of A, in CSR order, with the
        reference's rounding (sextans_sddmm_device_rm); d_vals_in may be None."""

    @_entry(f, p, p)
    def row_softmax_device(self, scale, d_x, d_p, stream=None):
        """p = softmax(scale * x) over the stored entries of every row of A (sextans_row_softmax_device): nnz floats each, in CSR entry
        order -- what sddmm_device_rm writes and update_values_device reads; d_p may be d_x."""

    @_entry(f, p, p, p)
    def row_softmax_backward_device(self, scale, d_p, d_g, d_dx, stream=None):
        """dx = scale * p * (g - sum_row p g) (sextans_row_softmax_backward_device); d_dx may be d_g or d_p."""

    @_entry(i, i, i, f, p, l, p, l, p, l, p, p, l, p)
    def attention_device(self, heads, d, dv, scale, d_Q, ldq, d_K, ldk, d_V, ldv, d_bias, d_O, ldo, d_lse, stream=None):
        """Fused multi-head attention on A's pattern (sextans_attention_device): O[r, h, :] = softmax_e(scale * (<Q[r, h, :], K[c, h, :]> +
        bias_e)) V[c, h, :] over the stored entries e = (r, c) of row r, lse[r, h] the row's log-sum-exp (M * heads floats).  Heads lie side
        by side in a row (a contiguous (rows, heads, d) tensor); d_bias: None, or nnz floats in CSR entry order shared by all heads.  A's
        own values are not read."""

    @_entry(*_frame("attention_device"), p, l, p, p, l, p, l, p, l, p)
    def attention_backward_device(self, heads, d, dv, scale, d_Q, ldq, d_K, ldk, d_V, ldv, d_bias, d_O, ldo, d_lse, d_G, ldg, d_delta,
                                  d_dQ, lddq, d_dK, lddk, d_dV, lddv, d_dbias, stream=None):
        """dQ, dK, dV (and, d_dbias not None, the bias gradient: nnz floats) of attention_device from its O and lse and the upstream
        gradient G (sextans_attention_backward_device); d_delta: M * heads floats of workspace the call writes."""

    @_entry(i, i, f, p, l, p, l, p, l, p, p, l, p)
    def gat_attention_device(self, heads, dv, negative_slope, d_adst, ldadst, d_asrc, ldasrc, d_V, ldv, d_bias, d_O, ldo, d_lse, stream=None):
        """Fused graph attention on A's pattern (sextans_gat_attention_device): O[r, h, :] = softmax_e(LeakyReLU((adst[r, h] + asrc[c, h]) +
        bias_e)) V[c, h, :] over the stored entries e = (r, c) of row r, lse[r, h] the row's log-sum-exp (M * heads floats).  adst is
        M x heads, asrc K x heads (ld >= heads), V K x (heads * dv) with the heads side by side; d_bias: None, or nnz floats in CSR entry
        order shared by all heads.  A's own values are not read."""

    @_entry(*_frame("gat_attention_device"), p, l, p, p, l, p, l, p, l, p)
    def gat_attention_backward_device(self, heads, dv, negative_slope, d_adst, ldadst, d_asrc, ldasrc, d_V, ldv, d_bias, d_O, ldo, d_lse, d_G, ldg,
                                      d_delta, d_dadst, lddadst, d_dasrc, lddasrc, d_dV, lddv, d_dbias, stream=None):
        """dadst, dasrc, dV (and, d_dbias not None, the bias gradient: nnz floats) of gat_attention_device from its O and lse and the
        upstream gradient G (sextans_gat_attention_backward_device); d_delta: M * heads floats of workspace the call writes."""

    @_entry(i, i, result=l)
    def gatv2_workspace_floats(self, heads, d):
        """Floats of workspace gatv2_attention_backward_device needs on this matrix (sextans_gatv2_workspace_floats):
        M * heads * d for datt_rows plus ceil(M / 256) * heads * d for the chunk sums."""

    @_entry(i, i, f, p, l, p, l, p, p, p, l, p)
    def gatv2_attention_device(self, heads, d, negative_slope, d_xdst, ldxd, d_xsrc, ldxs, d_att, d_bias, d_O, ldo, d_lse, stream=None):
        """Fused GATv2 attention on A's pattern (sextans_gatv2_attention_device): O[r, h, :] = softmax_e(<att[h, :], LeakyReLU(x_dst[r, h, :] +
        x_src[c, h, :])> + bias_e) x_src[c, h, :] over the stored entries e = (r, c) of row r, lse[r, h] the row's log-sum-exp (M * heads
        floats).  x_dst is M x (heads * d), x_src K x (heads * d) with the heads side by side, att heads * d floats; d_bias: None, or nnz
        floats in CSR entry order shared by all heads.  A's own values are not read."""

    @_entry(*_frame("gatv2_attention_device"), p, l, p, p, l, p, l, p, p, p)
    def gatv2_attention_backward_device(self, heads, d, negative_slope, d_xdst, ldxd, d_xsrc, ldxs, d_att, d_bias, d_O, ldo, d_lse, d_G, ldg,
                                        d_delta, d_dxdst, lddxd, d_dxsrc, lddxs, d_datt, d_work, d_dbias, stream=None):
        """dx_dst, dx_src, datt (heads * d floats, summed over the rows in a fixed two-level order) and, d_dbias not None, the bias gradient
        of gatv2_attention_device from its O and lse and the upstream gradient G (sextans_gatv2_attention_backward_device); d_delta:
        M * heads floats, d_work: gatv2_workspace_floats(heads, d) floats of workspace the call writes (datt_rows, then the chunk sums)."""

    # Attention dropout (sextans_*_dropout_device): the entries above with `drop`, a Dropout or None, before the stream.  drop None or
    # drop.p == 0: exactly the entry above.  The backward call takes the Dropout of its forward.
    @_entry(*_frame("attention_device"), ref(Dropout))
    def attention_dropout_device(self, heads, d, dv, scale, d_Q, ldq, d_K, ldk, d_V, ldv, d_bias, d_O, ldo, d_lse, drop, stream=None):
        ...

    @_entry(*_frame("attention_backward_device"), ref(Dropout))
    def attention_dropout_backward_device(self, heads, d, dv, scale, d_Q, ldq, d_K, ldk, d_V, ldv, d_bias, d_O, ldo, d_lse, d_G, ldg, d_delta,
                                          d_dQ, lddq, d_dK, lddk, d_dV, lddv, d_dbias, drop, stream=None):
        ...

    @_entry(*_frame("gat_attention_device"), ref(Dropout))
    def gat_attention_dropout_device(self, heads, dv, negative_slope, d_adst, ldadst, d_asrc, ldasrc, d_V, ldv, d_bias, d_O, ldo, d_lse, drop,
                                     stream=None):
        ...

    @_entry(*_frame("gat_attention_backward_device"), ref(Dropout))
    def gat_attention_dropout_backward_device(self, heads, dv, negative_slope, d_adst, ldadst, d_asrc, ldasrc, d_V, ldv, d_bias, d_O, ldo, d_lse,
                                              d_G, ldg, d_delta, d_dadst, lddadst, d_dasrc, lddasrc, d_dV, lddv, d_dbias, drop, stream=None):
        ...

    @_entry(*_frame("gatv2_attention_device"), ref(Dropout))
    def gatv2_attention_dropout_device(self, heads, d, negative_slope, d_xdst, ldxd, d_xsrc, ldxs, d_att, d_bias, d_O, ldo, d_lse, drop,
                                       stream=None):
        ...

    @_entry(*_frame("gatv2_attention_backward_device"), ref(Dropout))
    def gatv2_attention_dropout_backward_device(self, heads, d, negative_slope, d_xdst, ldxd, d_xsrc, ldxs, d_att, d_bias, d_O, ldo, d_lse, d_G,
                                                ldg, d_delta, d_dxdst, lddxd, d_dxsrc, lddxs, d_datt, d_work, d_dbias, drop, stream=None):
        ...

    @_entry(i, ref(Dropout), p)
    def dropout_mask_device(self, heads, drop, d_mult, stream=None):
        """The nnz * heads dropout multipliers of this matrix, [e * heads + h]: 1 / (1 - p) where (entry, head) is kept, 0 where it is
        dropped (sextans_dropout_mask_device) -- what the fused dropout kernels recompute."""

    @_entry(i, i, p, p, l, p, l, p, l)
    def spmm_reduce_device_rm(self, op, N, d_val, d_B, ldb, d_C, ldc, d_arg, ldarg, stream=None):
        """Max / min aggregation (sextans_spmm_reduce_device_rm): C[r, n] = max (REDUCE_MAX) or min (REDUCE_MIN) over row r's stored
        entries e = (r, c) of d_val[e] * B[c, n], arg[r, n] (int32; d_arg None: not written) the winning entry's position in the CSR
        arrays -- first of equal products, first NaN; an empty row gives +0 and -1.  d_val: nnz floats in entry order, None = the
        engine's current values.  B, C and arg row-major, N % 8 == 0."""

    @_entry(i, p, p, l, p, l, p, l, p, l, p)
    def spmm_reduce_backward_device_rm(self, N, d_val, d_B, ldb, d_arg, ldarg, d_G, ldg, d_dB, lddb, d_dval, stream=None):
        """dB (K x N) and dval (nnz floats) of spmm_reduce_device_rm from its arg and the upstream gradient G
        (sextans_spmm_reduce_backward_device_rm): every position's gradient goes to the entry that won it.  d_dB or d_dval may be
        None (not both); d_B may be None when d_dval is."""

    @_entry(i, p, p, l, ref(MultiOut))
    def spmm_multi_device_rm(self, N, d_val, d_B, ldb, out, stream=None):
        """Several aggregations of the messages d_val[e] * B[c, n] in one pass (sextans_spmm_multi_device_rm): out is a MultiOut whose
        given addresses receive the sum, the sum of squares, the max and the min over every row's entries (and the int32 args of the
        extrema, with the bits of spmm_reduce_device_rm); an empty row gives +0 and -1.  d_val None = the engine's current values."""

    @_entry(i, p, p, l, ref(MultiGrad), p, l, p)
    def spmm_multi_backward_device_rm(self, N, d_val, d_B, ldb, g, d_dB, lddb, d_dval, stream=None):
        """dB (K x N) and dval (nnz floats) of spmm_multi_device_rm from the upstream gradients and the args in g, a MultiGrad
        (sextans_spmm_multi_backward_device_rm): one column pass over A^T, one row pass over A.  d_dB or d_dval may be None (not both);
        d_B may be None when neither g.d_gsumsq nor d_dval is given."""

    @_entry(i, p, p, l, p, p, l, p, l)
    def spmm_softagg_device_rm(self, N, d_val, d_B, ldb, d_t, d_C, ldc, d_lse, ldlse, stream=None):
        """Softmax aggregation (sextans_spmm_softagg_device_rm): C[r, n] = sum over row r's stored entries e = (r, c) of
        softmax_e(t[n] * p_e[n]) * p_e[n], p_e[n] = d_val[e] * B[c, n] -- a softmax per column over the row's messages; lse[r, n] its
        log-sum-exp (d_lse None: not written).  d_t: N floats, None = 1; d_val None = the engine's current values.  An empty row gives +0
        and -inf.  B, C and lse row-major, N % 8 == 0."""

    @_entry(i, result=l)
    def spmm_softagg_workspace_floats(self, N):
        """Floats of workspace spmm_softagg_backward_device_rm needs for dt on this matrix (sextans_spmm_softagg_workspace_floats):
        M * N for the rows' sums plus ceil(M / 256) * N for the chunk sums."""

    @_entry(*_frame("spmm_softagg_device_rm"), p, l, p, l, p, p, p)
    def spmm_softagg_backward_device_rm(self, N, d_val, d_B, ldb, d_t, d_C, ldc, d_lse, ldlse, d_G, ldg, d_dB, lddb, d_dval, d_dt, d_work,
                                        stream=None):
        """dB (K x N), dval (nnz floats) and dt (N floats, summed over the rows in a fixed two-level order) of spmm_softagg_device_rm from
        its C and lse and the upstream gradient G (sextans_spmm_softagg_backward_device_rm).  Any of d_dB, d_dval, d_dt may be None (not
        all three); d_dt needs d_work, spmm_softagg_workspace_floats(N) floats the call writes."""

    @_entry(i, i, p, l, p, l, p, l)
    def spmm_edge_device_rm(self, op, N, d_B, ldb, d_E, lde, d_C, ldc, stream=None):
        """SpMM with a feature vector per stored entry (sextans_spmm_edge_device_rm): C[r, n] = sum over row r's entries e = (r, c) of
        B[c, n] * E[e, n] (EDGE_MUL), B + E (EDGE_ADD), relu(B + E) (EDGE_ADD_RELU) or E[e, n] (EDGE_COPY: d_B may be None).  Only the
        pattern is used; E is (nnz, N) row-major in the CSR entry order.  B, E and C row-major, N % 8 == 0; an empty row gives +0."""

    @_entry(i, i, p, l, p, l, p, l, p, l, p, l)
    def spmm_edge_backward_device_rm(self, op, N, d_B, ldb, d_E, lde, d_G, ldg, d_dB, lddb, d_dE, ldde, stream=None):
        """dB (K x N) and dE (nnz x N) of spmm_edge_device_rm from the upstream gradient G (sextans_spmm_edge_backward_device_rm): a
        column pass over A^T and a row pass over A, no atomics.  d_dB or d_dE may be None (not both; d_dB must be None with EDGE_COPY);
        d_B / d_E may be None where the op's gradient does not read them."""

    @_entry(*_frame("spmm_edge_device_rm"))
    def spmm_edge_device_rm_bf16(self, op, N, d_B, ldb, d_E, lde, d_C, ldc, stream=None):
        """spmm_edge_device_rm with E in bf16 (sextans_spmm_edge_device_rm_bf16): B and C fp32, E widened exactly -- the bits of
        spmm_edge_device_rm on the widened E.  lde counts bf16 elements (a multiple of 4)."""

    @_entry(*_frame("spmm_edge_backward_device_rm"))
    def spmm_edge_backward_device_rm_bf16(self, op, N, d_B, ldb, d_E, lde, d_G, ldg, d_dB, lddb, d_dE, ldde, stream=None):
        """spmm_edge_backward_device_rm with E and dE in bf16 (sextans_spmm_edge_backward_device_rm_bf16): B, G and dB fp32; dB the bits
        of spmm_edge_backward_device_rm on the widened E, dE its dE rounded once to nearest even.  lde and ldde count bf16 elements."""

    @_entry(i, i, p, l, p, l, p, p, l, p, l)
    def spmm_edge_softagg_device_rm(self, op, N, d_B, ldb, d_E, lde, d_t, d_C, ldc, d_lse, ldlse, stream=None):
        """Softmax aggregation of edge-feature messages (sextans_spmm_edge_softagg_device_rm): C[r, n] = sum over row r's stored entries
        e = (r, c) of softmax_e(t[n] * m_e[n]) * m_e[n], with the message m_e of spmm_edge_device_rm (B[c, n] * E[e, n], B + E, relu(B + E)
        or E[e, n] by op: EDGE_*; d_B may be None with EDGE_COPY) and the softmax per output column of spmm_softagg_device_rm; d_lse (may
        be None) gets log sum_e exp(t[n] m_e[n]).  Only A's pattern is read.  d_t: N temperatures, or None for 1.  An empty row: 0 and
        -inf.  N: a multiple of 8."""

    @_entry(i, result=l)
    def spmm_edge_softagg_workspace_floats(self, N):
        """Floats of workspace spmm_edge_softagg_backward_device_rm needs for dt on this matrix
        (sextans_spmm_edge_softagg_workspace_floats): M * N + ceil(M / 256) * N."""

    @_entry(*_frame("spmm_edge_softagg_device_rm"), p, l, p, l, p, l, p, p)
    def spmm_edge_softagg_backward_device_rm(self, op, N, d_B, ldb, d_E, lde, d_t, d_C, ldc, d_lse, ldlse, d_G, ldg, d_dB, lddb, d_dE, ldde,
                                             d_dt, d_work, stream=None):
        """dB (K x N), dE (nnz x N) and dt (N floats, summed over the rows in a fixed two-level order) of spmm_edge_softagg_device_rm from
        its C and lse and the upstream gradient G (sextans_spmm_edge_softagg_backward_device_rm): a column pass over A^T for dB, a row pass
        over A that stores dE and the rows' share of dt, no atomics.  Any of d_dB, d_dE, d_dt may be None (not all three; d_dB must be
        with EDGE_COPY); d_dt needs d_work, spmm_edge_softagg_workspace_floats(N) floats the call writes."""

    @_entry(i, i, p, l, p, l, p, l, p, l, p, l)
    def vector_attention_device_rm(self, msg, N, d_S, lds, d_V, ldv, d_D, ldd, d_C, ldc, d_lse, ldlse, stream=None):
        """Channel-wise attention from per-channel scores (sextans_vector_attention_device_rm): C[r, n] = sum over row r's stored entries
        e = (r, c) of softmax_e(S[e, n]) * m_e[n], a softmax per output column over the row's scores, which are READ from the (nnz, N)
        tensor S in A's entry order; the message m_e is V[c, n] (VATT_NODE), V[c, n] + D[e, n] (VATT_ADD) or D[e, n] (VATT_EDGE); the
        operand a mode does not read is ignored and may be None.  d_lse (may be None) gets log sum_e exp(S[e, n]).  Only A's pattern is
        read.  A score of -inf masks its (entry, column).  An empty row: 0 and -inf.  N: a multiple of 8."""

    @_entry(*_frame("vector_attention_device_rm"), p, l, p, l, p, l, p, l)
    def vector_attention_backward_device_rm(self, msg, N, d_S, lds, d_V, ldv, d_D, ldd, d_C, ldc, d_lse, ldlse, d_G, ldg, d_dS, ldds, d_dV,
                                            lddv, d_dD, lddd, stream=None):
        """dS (nnz x N), dV (K x N) and dD (nnz x N) of vector_attention_device_rm from its C and lse and the upstream gradient G
        (sextans_vector_attention_backward_device_rm): a row pass over A that stores dS and dD when either is given, a column pass over
        A^T for dV when it is given, no atomics.  Any of the three may be None, not all; d_dV must be None with VATT_EDGE, d_dD with
        VATT_NODE."""

    @_entry(*_frame("vector_attention_device_rm"))
    def vector_attention_device_rm_bf16(self, msg, N, d_S, lds, d_V, ldv, d_D, ldd, d_C, ldc, d_lse, ldlse, stream=None):
        """vector_attention_device_rm with S and D in bf16 (sextans_vector_attention_device_rm_bf16): V, C and lse fp32, S and D widened
        exactly (a bf16 -inf score still masks) -- the bits of vector_attention_device_rm on the widened S and D.  lds and ldd count bf16
        elements (multiples of 4)."""

    @_entry(*_frame("vector_attention_backward_device_rm"))
    def vector_attention_backward_device_rm_bf16(self, msg, N, d_S, lds, d_V, ldv, d_D, ldd, d_C, ldc, d_lse, ldlse, d_G, ldg, d_dS, ldds,
                                                 d_dV, lddv, d_dD, lddd, stream=None):
        """vector_attention_backward_device_rm with S, D, dS and dD in bf16 (sextans_vector_attention_backward_device_rm_bf16): V, C, lse,
        G and dV fp32; dV the bits of vector_attention_backward_device_rm on the widened S and D, dS and dD its dS and dD rounded once to
        nearest even.  lds, ldd, ldds and lddd count bf16 elements."""

    @_entry(*_frame("spmm_edge_softagg_device_rm"))
    def spmm_edge_softagg_device_rm_bf16(self, op, N, d_B, ldb, d_E, lde, d_t, d_C, ldc, d_lse, ldlse, stream=None):
        """spmm_edge_softagg_device_rm with E in bf16 (sextans_spmm_edge_softagg_device_rm_bf16): B, t, C and lse fp32, E widened exactly
        -- the bits of spmm_edge_softagg_device_rm on the widened E.  lde counts bf16 elements (a multiple of 4)."""

    @_entry(*_frame("spmm_edge_softagg_backward_device_rm"))
    def spmm_edge_softagg_backward_device_rm_bf16(self, op, N, d_B, ldb, d_E, lde, d_t, d_C, ldc, d_lse, ldlse, d_G, ldg, d_dB, lddb, d_dE,
                                                  ldde, d_dt, d_work, stream=None):
        """spmm_edge_softagg_backward_device_rm with E and dE in bf16 (sextans_spmm_edge_softagg_backward_device_rm_bf16): everything else
        fp32, the workspace that of spmm_edge_softagg_workspace_floats(N); dB and dt the bits of spmm_edge_softagg_backward_device_rm on
        the widened E, dE its dE rounded once to nearest even.  lde and ldde count bf16 elements."""

    @_entry(i, i, p, l, p, l, p, l, p, l)
    def edge_op_device_rm(self, op, N, d_xdst, ldxdst, d_xsrc, ldxsrc, d_E, lde, d_Z, ldz, stream=None):
        """Edge-output op from both endpoints (sextans_edge_op_device_rm): for every stored entry e = (r, c), in the CSR entry order,
        Z[e, n] = xdst[r, n] + / - / * xsrc[c, n] (EDGEOP_ADD / EDGEOP_SUB / EDGEOP_MUL), xdst[r, n] (EDGEOP_DST) or xsrc[c, n]
        (EDGEOP_SRC), one rounded fp32 operation, plus E[e, n] (a second rounded add) when d_E is given.  The operand an op does not read
        is ignored and may be None.  Only A's pattern is read.  N: a multiple of 8."""

    @_entry(i, i, p, l, p, l, p, l, p, l, p, l)
    def edge_op_backward_device_rm(self, op, N, d_xdst, ldxdst, d_xsrc, ldxsrc, d_Gz, ldgz, d_dxdst, lddxdst, d_dxsrc, lddxsrc, stream=None):
        """dxdst (M x N) and dxsrc (K x N) of edge_op_device_rm from the upstream gradient Gz of Z (sextans_edge_op_backward_device_rm):
        a sum over every row's entries and the same pass over A^T's rows, no atomics; dE is Gz itself.  Either may be None (not both;
        d_dxdst must be None with EDGEOP_SRC, d_dxsrc with EDGEOP_DST): its pass is skipped, and without d_dxsrc A^T is never built.
        xsrc is read only for EDGEOP_MUL's dxdst, xdst only for EDGEOP_MUL's dxsrc."""

    @_entry(*_frame("edge_op_device_rm"))
    def edge_op_device_rm_bf16(self, op, N, d_xdst, ldxdst, d_xsrc, ldxsrc, d_E, lde, d_Z, ldz, stream=None):
        """edge_op_device_rm with E (optional) and Z in bf16 (sextans_edge_op_device_rm_bf16): xdst and xsrc fp32, E widened exactly, the
        same fp32 operations, Z rounded once to nearest even -- round_bf16 of edge_op_device_rm's Z on the widened E.  lde and ldz count
        bf16 elements (multiples of 4)."""

    @_entry(*_frame("edge_op_backward_device_rm"))
    def edge_op_backward_device_rm_bf16(self, op, N, d_xdst, ldxdst, d_xsrc, ldxsrc, d_Gz, ldgz, d_dxdst, lddxdst, d_dxsrc, lddxsrc,
                                        stream=None):
        """edge_op_backward_device_rm with Gz in bf16 (sextans_edge_op_backward_device_rm_bf16): dxdst and dxsrc fp32, the bits of
        edge_op_backward_device_rm on the widened Gz.  ldgz counts bf16 elements (a multiple of 4)."""

    @_entry(i, i, p, l, p, l, p, l)
    def edge_dot_device(self, heads, d, d_X, ldx, d_Y, ldy, d_S, lds, stream=None):
        """Per-head dot product of both endpoints (sextans_edge_dot_device, DGL's u_dot_v): for every stored entry e = (r, c), in the CSR
        entry order, and every head h, S[e * lds + h] = sum_n X[r, h, n] * Y[c, h, n], every product and sum rounded to fp32 in column
        order (sddmm_device_rm's bits on the head's slice), all heads in one launch dealt by non-zeros.  X is M x heads*d, Y K x heads*d
        (score_attention_device's operands), d a multiple of 8 in [8, 128].  Only A's pattern is read."""

    @_entry(i, i, p, l, p, l, p, l, p, l, p, l)
    def edge_dot_backward_device(self, heads, d, d_X, ldx, d_Y, ldy, d_Gs, ldgs, d_dX, lddx, d_dY, lddy, stream=None):
        """dX (M x heads*d) and dY (K x heads*d) of edge_dot_device from the upstream gradient Gs of S (sextans_edge_dot_backward_device):
        score_attention_device(SCORE_WEIGHT)'s O with S := Gs, V := Y, and score_attention_backward_device(SCORE_WEIGHT)'s dV with S := Gs,
        G := X, no atomics.  Either may be None (not both): its pass is skipped, and without d_dY A^T is never built.  X is read only
        for dY, Y only for dX."""

    @_entry(i, f, i, ref(GatedIn), p, l, p, l, p, l)
    def spmm_gated_device_rm(self, mode, eps, N, gin, d_C, ldc, d_den, ldden, d_z, ldz, stream=None):
        """Gated aggregation (sextans_spmm_gated_device_rm): for the stored entry e = (r, c), z_e = (xdst[r] + xsrc[c]) + E[e] and
        g_e = sigmoid(z_e) per column; C[r] = sum_e g_e * V[c] (GATE_SUM) or that sum / (sum_e g_e + eps) (GATE_NORM).  gin: a GatedIn
        (d_e None: no edge features).  d_den (M x N; the gates' sums) and d_z (nnz x N in the CSR entry order; the new edge features)
        may be None.  Only the pattern is used; everything row-major, N % 8 == 0; an empty row gives +0."""

    @_entry(i, i, result=l)
    def spmm_gated_workspace_floats(self, mode, N):
        """Floats of workspace spmm_gated_backward_device_rm needs on this matrix (sextans_spmm_gated_workspace_floats): M * N in
        GATE_NORM mode (gn = G / (den + eps)), 0 in GATE_SUM mode."""

    @_entry(i, f, i, ref(GatedIn), p, l, p, l, p, l, p, l, ref(GatedGrad), p)
    def spmm_gated_backward_device_rm(self, mode, eps, N, gin, d_C, ldc, d_den, ldden, d_G, ldg, d_Gz, ldgz, out, d_work, stream=None):
        """The gradients of spmm_gated_device_rm named in out, a GatedGrad (sextans_spmm_gated_backward_device_rm): dxdst (M x N) and dE
        (nnz x N) from a row pass over A, dxsrc and dV (K x N) from a column pass over A^T; the gates are recomputed, no atomics.  d_G is
        the upstream gradient of C, d_Gz (None: absent) that of z.  d_C and d_den: the forward's, needed in GATE_NORM mode only, as is
        d_work, spmm_gated_workspace_floats(mode, N) floats the call writes."""

    @_entry(*_frame("spmm_gated_device_rm"))
    def spmm_gated_device_rm_bf16(self, mode, eps, N, gin, d_C, ldc, d_den, ldden, d_z, ldz, stream=None):
        """spmm_gated_device_rm with E and z in bf16 (sextans_spmm_gated_device_rm_bf16): gin a GatedIn whose d_e addresses bf16 (the
        struct's layout serves both), xdst, xsrc, V, C and den fp32.  E is widened exactly and the gate taken from the unrounded z -- C
        and den are the bits of spmm_gated_device_rm on the widened E, z its z rounded once to nearest even.  ld_e and ldz count bf16
        elements (multiples of 4)."""

    @_entry(*_frame("spmm_gated_backward_device_rm"))
    def spmm_gated_backward_device_rm_bf16(self, mode, eps, N, gin, d_C, ldc, d_den, ldden, d_G, ldg, d_Gz, ldgz, out, d_work, stream=None):
        """spmm_gated_backward_device_rm with E, Gz and dE in bf16 (sextans_spmm_gated_backward_device_rm_bf16): gin a GatedIn and out a
        GatedGrad whose d_e / d_de address bf16; everything else fp32, the workspace that of spmm_gated_workspace_floats(mode, N).  dxdst,
        dxsrc and dV are the bits of spmm_gated_backward_device_rm on the widened E and Gz, dE its dE rounded once to nearest even.  ld_e,
        ldgz and ld_de count bf16 elements."""

    @_entry(i, i, p, l, p, l, ref(MultiOut))
    def spmm_edge_multi_device_rm(self, op, N, d_B, ldb, d_E, lde, out, stream=None):
        """Several aggregations of edge-feature messages in one pass (sextans_spmm_edge_multi_device_rm): the message of the stored entry
        e = (r, c) is that of spmm_edge_device_rm (B[c, n] * E[e, n], B + E, relu(B + E) or E[e, n] by op: EDGE_*; d_B may be None with
        EDGE_COPY); out is a MultiOut whose given addresses receive the sum, the sum of squares, the max and the min over every row's
        entries and the int32 entry positions of the extrema; an empty row gives +0 and -1.  Only the pattern is used."""

    @_entry(i, i, p, l, p, l, ref(MultiGrad), p, l, p, l)
    def spmm_edge_multi_backward_device_rm(self, op, N, d_B, ldb, d_E, lde, g, d_dB, lddb, d_dE, ldde, stream=None):
        """dB (K x N) and dE (nnz x N) of spmm_edge_multi_device_rm from the upstream gradients and the args in g, a MultiGrad
        (sextans_spmm_edge_multi_backward_device_rm): a column pass over A^T and a row pass over A, no atomics.  d_dB or d_dE may be None
        (not both; d_dB must be None with EDGE_COPY); d_E is always needed, d_B unless EDGE_COPY."""

    @_entry(i, i, i, f, p, l, p, l, p, l, p, l, p, l, p, p, l, p, ref(Dropout))
    def attention_edge_device(self, heads, d, dv, scale, d_Q, ldq, d_K, ldk, d_V, ldv, d_Ek, ldek, d_Ev, ldev, d_bias, d_O, ldo, d_lse,
                              drop=None, stream=None):
        """Fused attention with a feature vector per stored entry on the key and on the value side (sextans_attention_edge_device):
        s_e = scale * (<Q[r, h, :], K[c, h, :] + Ek[e, h, :]> + bias_e), O[r, h, :] = sum_e softmax_e(s) (V[c, h, :] + Ev[e, h, :]).
        Ek is (nnz, heads * d), Ev (nnz, heads * dv), row-major in the CSR entry order; either may be None (no edge term on that side;
        both None: attention_dropout_device).  drop: a Dropout or None."""

    @_entry(i, i, i, f, p, l, p, l, p, l, p, l, p, l, p, p, l, p, p, l, p, p, l, p, l, p, l, p, l, p, l, p, ref(Dropout))
    def attention_edge_backward_device(self, heads, d, dv, scale, d_Q, ldq, d_K, ldk, d_V, ldv, d_Ek, ldek, d_Ev, ldev, d_bias, d_O, ldo, d_lse,
                                       d_G, ldg, d_delta, d_dQ, lddq, d_dK, lddk, d_dV, lddv, d_dEk, lddek, d_dEv, lddev, d_dbias,
                                       drop=None, stream=None):
        """dQ, dK, dV, dEk (nnz x heads * d), dEv (nnz x heads * dv) and, d_dbias not None, the bias gradient of attention_edge_device
        from its O and lse and the upstream gradient G (sextans_attention_edge_backward_device).  d_dEk / d_dEv may each be None; the
        same address for both (both E given, d == dv, lddek == lddev) stores the sum dEk + dEv once.  drop: the Dropout of the forward."""

    @_entry(i, i, i, p, l, p, l, p, l, p, ref(Dropout))
    def score_attention_device(self, mode, heads, dv, d_S, lds, d_V, ldv, d_O, ldo, d_lse, drop=None, stream=None):
        """Attention from caller-supplied scores (sextans_score_attention_device).  S is (nnz, heads), element (e, h) at S[e * lds + h], in the
        CSR entry order.  SCORE_SOFTMAX: O[r, h, :] = sum_e softmax_e(S[:, h] over row r) V[c, h, :] and lse (M x heads);
        SCORE_WEIGHT: O[r, h, :] = sum_e S[e, h] V[c, h, :] (d_lse is not touched and may be None).  drop: a Dropout or None (SOFTMAX only)."""

    @_entry(i, i, i, p, l, p, l, p, l, p, p, l, p, l, p, l, ref(Dropout))
    def score_attention_backward_device(self, mode, heads, dv, d_S, lds, d_V, ldv, d_O, ldo, d_lse, d_G, ldg, d_dS, ldds, d_dV, lddv,
                                        drop=None, stream=None):
        """dS (nnz x heads, element (e, h) at dS[e * ldds + h]: one plain store each) and dV of score_attention_device from the upstream
        gradient G -- SCORE_SOFTMAX: and its O and lse; SCORE_WEIGHT: d_O and d_lse are not read and may be None
        (sextans_score_attention_backward_device).  d_dS or d_dV may be None (not both): that pass is skipped.  drop: the forward's."""

    def spmm_device_rows(self, N, alpha, d_B, ldb, beta, d_C_in, ldc_in, d_C_out, ldc_out, row_begin, row_end,
                         reuse_b_panels=False, stream=None):
        _check(lib().sextans_spmm_device_rows(self._h, N, alpha, d_B, ldb, beta, d_C_in, ldc_in, d_C_out,
                                              ldc_out, row_begin, row_end, 1 if reuse_b_panels else 0,
                                              stream), "spmm_device_rows")

    def profile_read(self):
        k, n, r = C.c_double(), C.c_int64(), C.c_double()
        _check(lib().sextans_profile_read(self._h, C.byref(k), C.byref(n), C.byref(r)),
               "profile_read")
        return k.value, n.value, r.value

    def profile_read_post(self):
        """(mean ns, launches) of what calls launched behind their SpMM kernel (the reordered form's C staging -> C pass)."""
        k, n = C.c_double(), C.c_int64()
        _check(lib().sextans_profile_read_post(self._h, C.byref(k), C.byref(n)), "profile_read_post")
        return k.value, n.value

    def phase_timing_read(self):
        out = (C.c_int64 * 8)()
        _check(lib().sextans_phase_timing_read(self._h, out), "phase_timing_read")
        return list(out)

    @_entry()
    def profile_reset(self):
        ...

    def last_kernel(self):
        return lib().sextans_last_kernel(self._h).decode()


def dropout_keep_host(first, count, heads, p, seed, step=0):
    """The attention-dropout mask on the host, no device needed (sextans_dropout_keep_host): a (count, heads) uint8 array, 1 where
    (entry first + i, head h) is kept."""
    keep = np.zeros((max(count, 0), max(heads, 0)), np.uint8)
    m64 = 0xFFFFFFFFFFFFFFFF
    _check(lib().sextans_dropout_keep_host(first, count, heads, p, int(seed) & m64, int(step) & m64, keep.ctypes.data if keep.size else None),
           "dropout_keep_host")
    return keep


def spmm_csr(M, N, K, NNZ, ALPHA, CSRRowPtr, CSRColIndex, CSRVal, mat_B, BETA, mat_C):
    """One-shot call with cpu_spmm_CSR's argument list (sparse_helper.h:262-272); in place."""
    _check(lib().sextans_spmm_csr(M, N, K, NNZ, ALPHA, _buf(CSRRowPtr, np.int32),
                                  _buf(CSRColIndex, np.int32), _buf(CSRVal, np.float32),
                                  _buf(mat_B, np.float32), BETA, mat_C), "spmm_csr")
    return mat_C


# ------------------------------------------------------------------ synthetic inputs

def gen_csr_host(M, K, mean_nnz, seed, r0=0, r1=None, bandwidth=0):
    L = lib()
    r1 = M if r1 is None else r1
    p, i, v = C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.POINTER(C.c_float)()
    nnz = C.c_int64()
    _check(L.sextans_gen_csr_host(M, K, mean_nnz, bandwidth, seed, r0, r1, p, i, v, C.byref(nnz)),
           "gen_csr_host")
    out = (_take(p, r1 - r0 + 1, np.int32), _take(i, nnz.value, np.int32),
           _take(v, nnz.value, np.float32))
    for q in (p, i, v):
        L.sextans_host_free(q)
    return out


def gen_csr_device(device, M, K, mean_nnz, seed, r0=0, r1=None, bandwidth=0):
    """-> (d_row_ptr, d_col_idx, d_val, nnz) raw device pointers (ints); free with device_free."""
    r1 = M if r1 is None else r1
    p, i, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
    nnz = C.c_int64()
    _check(lib().sextans_gen_csr_device(device, M, K, mean_nnz, bandwidth, seed, r0, r1, C.byref(p),
                                        C.byref(i), C.byref(v), C.byref(nnz)), "gen_csr_device")
    return p.value, i.value, v.value, nnz.value


def gen_fem3d_host(nx, ny, nz, dof, seed, r0=0, r1=None):
    L = lib()
    r1 = nx * ny * nz * dof if r1 is None else r1
    p, i, v = C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.POINTER(C.c_float)()
    nnz = C.c_int64()
    _check(L.sextans_gen_fem3d_host(nx, ny, nz, dof, seed, r0, r1, p, i, v, C.byref(nnz)), "gen_fem3d_host")
    out = (_take(p, r1 - r0 + 1, np.int32), _take(i, nnz.value, np.int32), _take(v, nnz.value, np.float32))
    for q in (p, i, v):
        L.sextans_host_free(q)
    return out


def device_alloc(device, nbytes):
    """hipMalloc through the library's own HIP runtime (free with device_free)."""
    ptr = C.c_void_p()
    _check(lib().sextans_device_alloc(device, nbytes, C.byref(ptr)), "device_alloc")
    return ptr.value


COPY_H2D, COPY_D2H, COPY_D2D = 1, 2, 3


def device_copy(device, dst, src, nbytes, kind=COPY_D2D):
    """Synchronous copy through the library's own HIP runtime (never a second dlopen of libamdhip64 by another name: where torch
    bundles its own copy that maps a second runtime, which fails on this one's pointers).  dst / src: integer addresses."""
    _check(lib().sextans_device_copy(device, C.c_void_p(dst), C.c_void_p(src), nbytes, kind), "device_copy")


def upload_csr(device, rp, ci, v):
    """Host CSR arrays -> device copies (torch allocations would be freed with their tensors; these are hipMalloc'ed through the
    library and freed with device_free).  Returns device pointers (rp, ci, v)."""
    out = []
    for arr, dt in ((rp, np.int32), (ci, np.int32), (v, np.float32)):
        a = np.ascontiguousarray(arr, dt)
        ptr = device_alloc(device, a.nbytes)
        if a.nbytes:
            device_copy(device, ptr, a.ctypes.data, a.nbytes, COPY_H2D)
        out.append(ptr)
    return tuple(out)


def permute_symmetric_device(device, M, nnz, d_rp, d_ci, d_v, new_of_old):
    """P A P^T on the device (row / column i -> new_of_old[i]); returns new device pointers (rp, ci, v) -- free with device_free."""
    p, i, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
    no = np.ascontiguousarray(new_of_old, np.int32)
    L = lib()
    _check(L.sextans_csr_permute_symmetric_device(device, M, nnz, d_rp, d_ci, d_v, no.ctypes.data, C.byref(p), C.byref(i), C.byref(v)),
           "csr_permute_symmetric_device")
    return p.value, i.value, v.value


def slice_rows_device(device, r0, r1, d_rp, d_ci, d_v):
    """Rows [r0, r1) of a device CSR matrix as (rp, ci, v, nnz): rp is a new device array (device_free), ci / v point INTO the originals."""
    p, first, nnz = C.c_void_p(), C.c_int64(), C.c_int64()
    L = lib()
    _check(L.sextans_csr_slice_rows_device(device, r0, r1, d_rp, C.byref(p), C.byref(first), C.byref(nnz)), "csr_slice_rows_device")
    return p.value, d_ci + 4 * first.value, d_v + 4 * first.value, nnz.value


def gen_fem3d_device(device, nx, ny, nz, dof, seed, r0=0, r1=None):
    r1 = nx * ny * nz * dof if r1 is None else r1
    p, i, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
    nnz = C.c_int64()
    _check(lib().sextans_gen_fem3d_device(device, nx, ny, nz, dof, seed, r0, r1, C.byref(p), C.byref(i),
                                          C.byref(v), C.byref(nnz)), "gen_fem3d_device")
    return p.value, i.value, v.value, nnz.value


def _gen_host(fn, args, nrows):
    L = lib()
    p, i, v = C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.POINTER(C.c_float)()
    nnz = C.c_int64()
    _check(fn(*args, p, i, v, C.byref(nnz)), fn.__name__)
    out = (_take(p, nrows + 1, np.int32), _take(i, nnz.value, np.int32), _take(v, nnz.value, np.float32))
    for q in (p, i, v):
        L.sextans_host_free(q)
    return out


def _gen_device(fn, args):
    p, i, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
    nnz = C.c_int64()
    _check(fn(*args, C.byref(p), C.byref(i), C.byref(v), C.byref(nnz)), fn.__name__)
    return p.value, i.value, v.value, nnz.value


def gen_stencil2d_host(nx, ny, points, dof, seed, r0=0, r1=None):
    """2-D stencil (5 or 9 points) on an nx x ny grid, dof unknowns per node -> (row_ptr, col_idx, val)."""
    r1 = nx * ny * dof if r1 is None else r1
    return _gen_host(lib().sextans_gen_stencil2d_host, (nx, ny, points, dof, seed, r0, r1), r1 - r0)


def gen_stencil2d_device(device, nx, ny, points, dof, seed, r0=0, r1=None):
    r1 = nx * ny * dof if r1 is None else r1
    return _gen_device(lib().sextans_gen_stencil2d_device, (device, nx, ny, points, dof, seed, r0, r1))


def kkt_rows(n, arrow):
    return n + n // 2 + arrow


def gen_kkt_host(n, arrow, seed, r0=0, r1=None):
    """KKT / arrow block structure (n variables, n/2 constraints, `arrow` border rows/columns) -> (row_ptr, col_idx, val)."""
    r1 = kkt_rows(n, arrow) if r1 is None else r1
    return _gen_host(lib().sextans_gen_kkt_host, (n, arrow, seed, r0, r1), r1 - r0)


def gen_kkt_device(device, n, arrow, seed, r0=0, r1=None):
    r1 = kkt_rows(n, arrow) if r1 is None else r1
    return _gen_device(lib().sextans_gen_kkt_device, (device, n, arrow, seed, r0, r1))


def gen_kron_host(n, p_rp, p_ci, pk, variant, seed, r0=0, r1=None):
    """kron(T_n, P) holdout class (include/sextans_amd.h) -> (row_ptr, col_idx, val, K)."""
    L = lib()
    p_rp = np.ascontiguousarray(p_rp, np.int32); p_ci = np.ascontiguousarray(p_ci, np.int32)
    pm = len(p_rp) - 1
    r1 = n * pm if r1 is None else r1
    p, i, v = C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.POINTER(C.c_float)()
    nnz, K = C.c_int64(), C.c_int()
    _check(L.sextans_gen_kron_host(n, pm, pk, p_rp, p_ci, variant, seed, r0, r1, C.byref(p), C.byref(i), C.byref(v), C.byref(nnz),
                                   C.byref(K)), "gen_kron_host")
    out = (_take(p, r1 - r0 + 1, np.int32), _take(i, nnz.value, np.int32), _take(v, nnz.value, np.float32), K.value)
    for q in (p, i, v):
        L.sextans_host_free(q)
    return out


def gen_kron_device(device, n, p_rp, p_ci, pk, variant, seed, r0=0, r1=None):
    """Device form -> (d_row_ptr, d_col_idx, d_val, nnz, K); free the arrays with device_free."""
    L = lib()
    p_rp = np.ascontiguousarray(p_rp, np.int32); p_ci = np.ascontiguousarray(p_ci, np.int32)
    pm = len(p_rp) - 1
    r1 = n * pm if r1 is None else r1
    p, i, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
    nnz, K = C.c_int64(), C.c_int()
    _check(L.sextans_gen_kron_device(device, n, pm, pk, p_rp, p_ci, variant, seed, r0, r1, C.byref(p), C.byref(i), C.byref(v),
                                     C.byref(nnz), C.byref(K)), "gen_kron_device")
    return p.value, i.value, v.value, nnz.value, K.value


def gen_powerlaw_host(M, K, xmin, tail_x100, max_len, seed, r0=0, r1=None):
    """Power-law row lengths, P(len >= x) = (xmin/x)^(tail_x100/100) on [xmin, max_len] -> (row_ptr, col_idx, val)."""
    L = lib()
    r1 = M if r1 is None else r1
    p, i, v = C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.POINTER(C.c_float)()
    nnz = C.c_int64()
    _check(L.sextans_gen_powerlaw_host(M, K, xmin, tail_x100, max_len, seed, r0, r1, p, i, v, C.byref(nnz)),
           "gen_powerlaw_host")
    out = (_take(p, r1 - r0 + 1, np.int32), _take(i, nnz.value, np.int32), _take(v, nnz.value, np.float32))
    for q in (p, i, v):
        L.sextans_host_free(q)
    return out


def gen_powerlaw_device(device, M, K, xmin, tail_x100, max_len, seed, r0=0, r1=None):
    r1 = M if r1 is None else r1
    p, i, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
    nnz = C.c_int64()
    _check(lib().sextans_gen_powerlaw_device(device, M, K, xmin, tail_x100, max_len, seed, r0, r1, C.byref(p),
                                             C.byref(i), C.byref(v), C.byref(nnz)), "gen_powerlaw_device")
    return p.value, i.value, v.value, nnz.value


def gen_bell_host(M, K, ell_width, seed):
    L = lib()
    c, v = C.POINTER(C.c_int)(), C.POINTER(C.c_uint16)()
    _check(L.sextans_gen_bell_host(M, K, ell_width, seed, c, v), "gen_bell_host")
    n = (M // 32) * ell_width
    out = (_take(c, n, np.int32), np.ctypeslib.as_array(v, shape=(n * 1024,)).astype(np.uint16, copy=True))
    L.sextans_host_free(c); L.sextans_host_free(v)
    return out


def gen_bell_device(device, M, K, ell_width, seed):
    c, v = C.c_void_p(), C.c_void_p()
    _check(lib().sextans_gen_bell_device(device, M, K, ell_width, seed, C.byref(c), C.byref(v)), "gen_bell_device")
    return c.value, v.value


def gen_bell_banded_host(M, K, half_width, seed):
    """Block-banded blocked-ELL (2 * half_width + 1 consecutive block columns per block row): block rows share columns."""
    L = lib()
    c, v = C.POINTER(C.c_int)(), C.POINTER(C.c_uint16)()
    _check(L.sextans_gen_bell_banded_host(M, K, half_width, seed, c, v), "gen_bell_banded_host")
    n = (M // 32) * (2 * half_width + 1)
    out = (_take(c, n, np.int32), np.ctypeslib.as_array(v, shape=(n * 1024,)).astype(np.uint16, copy=True))
    L.sextans_host_free(c); L.sextans_host_free(v)
    return out


def gen_bell_banded_device(device, M, K, half_width, seed):
    c, v = C.c_void_p(), C.c_void_p()
    _check(lib().sextans_gen_bell_banded_device(device, M, K, half_width, seed, C.byref(c), C.byref(v)), "gen_bell_banded_device")
    return c.value, v.value


def gen_uniform_bf16_host(n, seed):
    a = np.empty(max(n, 1), np.uint16)
    _check(lib().sextans_gen_uniform_bf16_host(a, n, seed), "gen_uniform_bf16_host")
    return a[:n]


def gen_uniform_bf16_device(device, d_ptr, n, seed, stream=None):
    _check(lib().sextans_gen_uniform_bf16_device(device, d_ptr, n, seed, stream), "gen_uniform_bf16_device")


def gen_uniform_host(n, seed):
    a = np.empty(max(n, 1), np.float32)
    _check(lib().sextans_gen_uniform_host(a, n, seed), "gen_uniform_host")
    return a[:n]


def gen_uniform_device(device, d_ptr, n, seed, stream=None):
    _check(lib().sextans_gen_uniform_device(device, d_ptr, n, seed, stream), "gen_uniform_device")


def partition_rows_by_nnz(row_ptr, world):
    """C-ABI twin of sextans_amd.dist.partition_rows_by_nnz: [(r0, r1)] * world."""
    rp = _buf(row_ptr, np.int32)
    out = np.zeros(2 * world, np.int32)
    _check(lib().sextans_partition_rows_by_nnz(len(rp) - 1, rp, world, out), "partition_rows_by_nnz")
    return [(int(out[2 * g]), int(out[2 * g + 1])) for g in range(world)]


def dist_bind_library(path=None):
    """Which library the collectives come from (None: the default RCCL search); sextans_dist_bind_library."""
    _check(lib().sextans_dist_bind_library(path.encode() if path else None), "sextans_dist_bind_library")


def dist_unique_id():
    """128-byte RCCL id (rank 0 creates it, the other ranks receive it by the caller's own means)."""
    buf = C.create_string_buffer(128)
    _check(lib().sextans_dist_unique_id(buf), "dist_unique_id")
    return buf.raw


def dist_comm_init(device, world, rank, uid):
    comm = C.c_void_p()
    _check(lib().sextans_dist_comm_init(C.byref(comm), device, world, rank, uid), "dist_comm_init")
    return comm


def dist_comm_destroy(comm):
    _check(lib().sextans_dist_comm_destroy(comm), "dist_comm_destroy")


def csr_transpose_device(device, M, K, nnz, d_rp, d_ci, d_v, stream=None):
    """CSR of A^T (K x M) as new device arrays (row_ptr, col_idx, val; free each with device_free), byte-identical to the reference's
    CSC_2_CSR of A's CSR read as the CSC of A^T (sextans_csr_transpose_device)."""
    p, i, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _check(lib().sextans_csr_transpose_device(device, M, K, nnz, d_rp, d_ci, d_v, C.byref(p), C.byref(i), C.byref(v), stream),
           "csr_transpose_device")
    return p.value, i.value, v.value


def device_free(device, d_ptr):
    _check(lib().sextans_device_free(device, d_ptr), "device_free")


# Every entry point added after round 4 -- the only ones an OLDER build may lack.  Derived: a new entry point is optional with no further edit.
_OPTIONAL_SYMBOLS = frozenset(_PROTOTYPES) - _ROUND4_SYMBOLS
