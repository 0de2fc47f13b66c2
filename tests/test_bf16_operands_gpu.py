"""bf16 dense operands on the row-major CSR entry (sextans_spmm_device_rm_bf16, sextans_spmm_t_device_rm_bf16, sextans_prepare_rm_bf16).

B is drawn as fp32 and rounded to bf16 by torch; the oracle (cpu_spmm_CSR restated) gets the widened values, so the expected fp32 result
is the oracle's and the expected bf16 result is torch's CPU rounding of it.  All comparisons are on bits, NaNs compared as NaNs.

One rule says which route a call must take, so that no test guesses at the dispatcher: a bf16 call is NATIVE iff the fp32 entry point,
called on the same engine with the widened operands, reports a last_kernel() that starts with "spmm_csr_rowgroup_rowmajor", stat
"exact_chain_rows" is 0 and the bf16 operands allow 16-byte accesses (16-byte aligned pointers, ldb % 8 == 0, C's ld % 4 == 0 for fp32 /
% 8 == 0 for bf16).  (The engine's predicate has one more term, which no test here reaches: B below 4 GB, K * ldb * 2 < 2^32 -- the
kernels address B with 32-bit byte offsets; a larger B converts.)  The counters "bf16_native_calls" / "bf16_converted_calls" say which one happened."""
import numpy as np
import pytest

from test_rowmajor_gpu import _matrices, _run as _run32, _want
from util import ALPHA, BETA, bits_equal, random_csr

pytestmark = pytest.mark.gpu

PAD_B, PAD_CIN, PAD_C = 7.0, 9.0, -5.0      # fill of the padding columns (all exact in bf16)
PAIRS = ((ALPHA, BETA), (0.0, 1.0), (1.0, 0.0), (0.0, 0.0))


def to_bf16(x32):
    """fp32 array -> bf16 bit patterns (uint16), rounded by torch on the CPU"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x32, np.float32)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def widen(b16):
    return (np.ascontiguousarray(b16, np.uint16).astype(np.uint32) << 16).view(np.float32)


def same16(a, b):
    a, b = np.ascontiguousarray(a, np.uint16), np.ascontiguousarray(b, np.uint16)
    na, nb = np.isnan(widen(a)), np.isnan(widen(b))
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb])


def counts(e):
    return int(e.get_stat("bf16_native_calls")), int(e.get_stat("bf16_converted_calls"))


def _buf(a, ld, off_bytes, fill):
    """(rows, cols) uint16 / float32 numpy -> device buffer with leading dimension ld whose first element lies off_bytes behind an
    allocation boundary; returns (flat tensor, (rows, ld) view, address of the first element)"""
    import torch
    rows, cols = a.shape
    esz = a.dtype.itemsize
    assert off_bytes % esz == 0 and ld >= cols
    head = off_bytes // esz
    if esz == 2:
        t = torch.full((rows * ld + head,), fill, dtype=torch.bfloat16, device="cuda").view(torch.int16)
        src = torch.from_numpy(np.ascontiguousarray(a).view(np.int16))
    else:
        t = torch.full((rows * ld + head,), fill, dtype=torch.float32, device="cuda")
        src = torch.from_numpy(np.ascontiguousarray(a))
    v = t[head:].view(rows, ld)
    v[:, :cols] = src.cuda()
    assert t.data_ptr() % 256 == 0
    return t, v, t.data_ptr() + off_bytes


def _host(v):
    a = v.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def run16(e, B16, C0, ldb=None, ldc_in=None, ldc=None, inplace=False, alpha=ALPHA, beta=BETA, offb=0, offc=0, transposed=False):
    """One call of the bf16 entry point.  B16: uint16 bit patterns; C0: uint16 (bf16 C) or float32 (fp32 C); off*: bytes by which the
    pointers miss an allocation boundary.  The padding columns of B, C_in and C_out must come back untouched."""
    import torch
    from sextans_amd import api
    rb, N = B16.shape
    rc = C0.shape[0]
    cbf16 = C0.dtype == np.uint16
    ldb, ldc_in, ldc = ldb or N, ldc_in or N, ldc or N
    tb, vb, pb = _buf(B16, ldb, offb, PAD_B)
    tci, vci, pci = _buf(C0, ldc_in, offc, PAD_CIN)
    if inplace:
        vco, pco, ldc = vci, pci, ldc_in
    else:
        tco, vco, pco = _buf(np.zeros((rc, 0), C0.dtype), ldc, offc, PAD_C)
    call = e.spmm_t_device_rm_bf16 if transposed else e.spmm_device_rm_bf16
    call(N, float(alpha), pb, ldb, float(beta), pci, ldc_in, pco, ldc, api.DTYPE_BF16 if cbf16 else api.DTYPE_F32,
         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    full = _host(vco)
    pad = to_bf16(np.float32([PAD_CIN if inplace else PAD_C]))[0] if cbf16 else np.float32(PAD_CIN if inplace else PAD_C)
    assert np.all(full[:, N:] == pad), "columns of C beyond N were written"
    assert np.all(_host(vb)[:, N:] == to_bf16(np.float32([PAD_B]))[0]), "padding of B was written"
    if not inplace:
        assert np.all(_host(vci)[:, N:] == (to_bf16(np.float32([PAD_CIN]))[0] if cbf16 else np.float32(PAD_CIN))) and \
            np.array_equal(_host(vci)[:, :N], C0), "C_in was written"
    return np.ascontiguousarray(full[:, :N])


def check(e, B16, C0, want32, native, **kw):
    """The call moves exactly one counter -- the one `native` names -- and returns want32 (fp32 C) or its rounding (bf16 C)"""
    n0, c0 = counts(e)
    got = run16(e, B16, C0, **kw)
    n1, c1 = counts(e)
    assert (n1 - n0, c1 - c0) == ((1, 0) if native else (0, 1)), (native, (n0, c0), (n1, c1), e.last_kernel(), kw)
    if C0.dtype == np.uint16:
        assert same16(got, to_bf16(want32)), (e.last_kernel(), kw)
    else:
        assert bits_equal(got, want32), (e.last_kernel(), kw)
    return got


def aligned(N, cbf16, ldb=None, ldc_in=None, ldc=None, inplace=False, offb=0, offc=0, **_):
    cm = 8 if cbf16 else 4
    ldb, ldc_in, ldc = ldb or N, ldc_in or N, ldc or N
    return offb % 16 == 0 and offc % 16 == 0 and ldb % 8 == 0 and ldc_in % cm == 0 and (inplace or ldc % cm == 0)


def rule(e, M, K, N, B32, c32, cbf16, alpha=ALPHA, beta=BETA, **kw):
    """-> (the bf16 call with these operands must be native, the fp32 entry's result on the widened operands)"""
    got32 = _run32(e, M, K, N, B32, c32, alpha=alpha, beta=beta)
    gather = e.last_kernel().startswith("spmm_csr_rowgroup_rowmajor") and e.get_stat("exact_chain_rows") == 0
    return bool(gather and aligned(N, cbf16, **kw)), got32


def big_random_csr(rs, M, K, mean):
    """random_csr without its per-row Python loop: sorted distinct columns, ~5 % empty rows"""
    lens = rs.poisson(mean, M)
    lens[rs.rand(M) < 0.05] = 0
    row = np.repeat(np.arange(M), lens)
    col = rs.randint(0, K, row.size)
    order = np.lexsort((col, row))
    row, col = row[order], col[order]
    keep = np.ones(row.size, bool)
    keep[1:] = (row[1:] != row[:-1]) | (col[1:] != col[:-1])
    row, col = row[keep], col[keep]
    rp = np.zeros(M + 1, np.int32)
    rp[1:] = np.cumsum(np.bincount(row, minlength=M))
    return rp, col.astype(np.int32), rs.uniform(-1, 1, col.size).astype(np.float32)


def operands(seed, rows_b, rows_c, N):
    rs = np.random.RandomState(seed)
    B16 = to_bf16(rs.uniform(-1, 1, (rows_b, N)))
    C32 = rs.uniform(-1, 1, (rows_c, N)).astype(np.float32)
    return B16, widen(B16), C32, to_bf16(C32)


@pytest.mark.parametrize("size", ["small", "large"])
def test_native_gather_path_strict(sx, oracle, size):
    """1. No B-row reuse (config 4's class): the bf16 gather kernel on the caller's buffers, both A-stream forms, every tile width and
    the 8-column tail, C fp32 and bf16, padded leading dimensions, in place, special alpha / beta: bit-identical to the oracle."""
    rs = np.random.RandomState(12)
    if size == "small":
        M, K = 5003, 7001                      # the matrix of test_rowmajor_gather_kernel
        rp, ci, v = random_csr(rs, M, K, 12)
    else:
        M, K = 200003, 150001
        rp, ci, v = big_random_csr(rs, M, K, 8)
    wants = {}
    with sx.Engine(0) as e:
        for stage in (1, 0):
            e.set_option("stage_a", stage)
            e.set_matrix_csr(M, K, rp, ci, v)
            total = 0
            for N in (8, 16, 24, 32, 64, 72, 128, 256):
                B16, B32, C32, C16 = operands(N, K, M, N)
                if N == 16:   # what the rule says about this matrix, for the record: the fp32 entry runs the gather kernel
                    assert rule(e, M, K, N, B32, C32, False)[0] and e.last_kernel() == "spmm_csr_rowgroup_rowmajor"
                for alpha, beta in PAIRS:
                    for cb in (False, True):
                        key = (N, float(alpha), float(beta), cb)
                        if key not in wants:
                            wants[key] = _want(oracle, M, K, N, rp, ci, v, B32, widen(C16) if cb else C32, np.float32(alpha), np.float32(beta))
                        kws = ({}, {"ldb": N + 8, "ldc_in": N + 16, "ldc": N + 16}, {"inplace": True}) if (alpha, beta) == PAIRS[0] else ({},)
                        for kw in kws:
                            check(e, B16, C16 if cb else C32, wants[key], True, alpha=alpha, beta=beta, **kw)
                            assert e.last_kernel() == "spmm_csr_rowgroup_rowmajor_bf16", (N, e.last_kernel())
                            total += 1
            assert counts(e) == (total, 0)      # (per matrix: set_matrix resets them)


def test_long_rows_native_and_exact_chains_converted(sx, oracle):
    """2. Bucketed long rows stay native (piece kernel + fold); exact chains convert; split hub rows of the fast mode are native again."""
    from sextans_amd import api
    rs = np.random.RandomState(11)
    M = K = 3000
    rp, ci, v = random_csr(rs, M, K, 10, long_rows=3)
    with sx.Engine(0) as e:
        e.set_matrix_csr(M, K, rp, ci, v)
        for N in (8, 24, 64, 72):
            B16, B32, C32, C16 = operands(N + 1, K, M, N)
            for cb in (False, True):
                c32 = widen(C16) if cb else C32
                want = _want(oracle, M, K, N, rp, ci, v, B32, c32)
                for kw in ({}, {"ldb": N + 8, "ldc_in": N + 16, "ldc": N + 16}, {"inplace": True}):
                    native, _ = rule(e, M, K, N, B32, c32, cb, **kw)
                    assert native and e.last_kernel() == "spmm_csr_rowgroup_rowmajor+long_rows", (N, e.last_kernel())
                    check(e, B16, C16 if cb else C32, want, True, **kw)
                    assert e.last_kernel() == "spmm_csr_rowgroup_rowmajor_bf16+long_rows", (N, e.last_kernel())
        assert e.get_stat("piece_path_rows") > 0 and counts(e)[1] == 0
    M = K = 20000
    rp, ci, v = api.gen_powerlaw_host(M, K, 3, 120, 15000, 11)
    for fast in (False, True):
        with sx.Engine(0) as e:
            if fast:
                e.set_option("mode", 1)
            e.set_matrix_csr(M, K, rp, ci, v)
            for N in (16, 40):
                B16, B32, C32, C16 = operands(N + 2, K, M, N)
                for cb in (False, True):
                    c32 = widen(C16) if cb else C32
                    native, got32 = rule(e, M, K, N, B32, c32, cb)
                    assert e.last_kernel() == "spmm_csr_rowgroup_rowmajor+long_rows", e.last_kernel()
                    want = _want(oracle, M, K, N, rp, ci, v, B32, c32)
                    if not fast:
                        assert e.get_stat("exact_chain_rows") > 0 and not native      # chains exist: the call converts
                        assert bits_equal(got32, want)
                    else:
                        assert e.get_stat("exact_chain_rows") == 0 and len(e.reassociated_rows()) > 0
                        # the header's bound for SEXTANS_MODE_FAST: 1e-4 * (|alpha| sum|a b| + |beta c|)
                        mag = _want(oracle, M, K, N, rp, ci, np.abs(v), np.abs(B32), np.zeros_like(c32), np.float32(1.0), np.float32(0.0))
                        bound = 1e-4 * (abs(float(ALPHA)) * mag.astype(np.float64) + np.abs(float(BETA) * c32.astype(np.float64))) + 1e-30
                        assert np.all(np.abs(got32.astype(np.float64) - want) <= bound)
                    # ... and whichever route: the bits of the fp32 entry point on the widened B
                    check(e, B16, C16 if cb else C32, got32, native)


def _route_cases():
    from sextans_amd import api
    from test_mixed_plan_gpu import _mixed_matrix
    for name, mat, _, opts in _matrices():
        yield name, mat, opts, {}
    rp, ci, v = api.gen_stencil2d_host(90, 81, 5, 1, 3)
    yield "5-point stencil, lane per row", (rp, ci, v, 7290, 7290), {}, {}
    yield "mixed plan", _mixed_matrix(), {}, {}
    rs = np.random.RandomState(11)
    rp, ci, v = random_csr(rs, 5000, 7000, 12)
    yield "gather class, pointers 2 (bf16) / 4 (fp32 C) bytes off", (rp, ci, v, 5000, 7000), {}, {"offb": 2, "offc": -1}
    yield "gather class, pointers 8 bytes off", (rp, ci, v, 5000, 7000), {}, {"offb": 8, "offc": 8}


@pytest.mark.parametrize("fast", [False, True])
def test_every_route_has_the_bits_of_the_fp32_entry(sx, fast):
    """3. Whatever the dispatcher picks -- LDS-panel plans (natural, grid bricks, graph-clustered), lane per row, a mixed plan,
    unaligned operands -- the bf16 entry returns what spmm_device_rm returns on the widened operands, bit for bit, in both modes and
    for both C types, and a bf16 C is the rounding of the fp32 C.  Exactly one counter moves per call: the one the rule names."""
    seen = set()
    for name, (rp, ci, v, M, K), opts, kw in _route_cases():
        with sx.Engine(0) as e:
            if fast:
                e.set_option("mode", 1)
            for k, val in opts.items():
                e.set_option(k, val)
            e.set_matrix_csr(M, K, rp, ci, v)
            for N in (24, 64):
                B16, B32, C32, C16 = operands(N + M % 7, K, M, N)
                for cb in (False, True):
                    c32 = widen(C16) if cb else C32
                    kw_c = dict(kw)
                    if kw_c.get("offc") == -1:
                        kw_c["offc"] = 2 if cb else 4
                    native, got32 = rule(e, M, K, N, B32, c32, cb, **kw_c)
                    seen.add((name, e.last_kernel()))
                    got = check(e, B16, C16 if cb else C32, got32, native, **kw_c)
                    if cb:
                        assert same16(got, to_bf16(got32)), (name, N)
                    assert not native, (name, N, e.last_kernel())       # (none of these is an aligned call on the gather path)
    kernels = {k for _, k in seen}
    assert any(k.startswith("spmm_csr_panel_v2_rowmajor_clustered") for k in kernels) and "spmm_csr_colwise_rowmajor" in kernels and \
        "spmm_csr_panel_v2_rowmajor" in kernels, seen


def test_transposed_form(sx, oracle):
    """4. spmm_t_device_rm_bf16 against cpu_spmm_CSR on CSC_2_CSR(A), on the companion engine: a gather-class matrix (native there)
    and an FEM matrix (converted)."""
    import torch
    from sextans_amd import api
    from test_spmm_transposed_gpu import run_t, want_t
    rs = np.random.RandomState(5)
    rp, ci, v = random_csr(rs, 6000, 5000, 11)
    cases = [("gather class", rp, ci, v, 6000, 5000)]
    rp, ci, v = api.gen_fem3d_host(14, 13, 12, 3, 7)
    cases.append(("fem", rp, ci, v, 14 * 13 * 12 * 3, 14 * 13 * 12 * 3))
    for name, rp, ci, v, M, K in cases:
        with sx.Engine(0) as e:
            e.set_matrix_csr(M, K, rp, ci, v)
            for N in (16, 40):
                B16, B32, C32, C16 = operands(N, M, K, N)             # B is M x N, C is K x N
                for cb in (False, True):
                    c32 = widen(C16) if cb else C32
                    want = want_t(oracle, M, K, rp, ci, v, B32, ALPHA, BETA, c32)
                    got32 = run_t(e, B32, ALPHA, BETA, c32)
                    native = e.last_kernel().startswith("spmm_csr_rowgroup_rowmajor")   # (no chains in either A^T)
                    assert bits_equal(got32, want) and native == (name == "gather class"), (name, e.last_kernel())
                    for kw in ({}, {"ldb": N + 8, "ldc_in": N + 16, "ldc": N + 16}, {"inplace": True}):
                        check(e, B16, C16 if cb else C32, want, native, transposed=True, **kw)
                    assert e.last_kernel().startswith("spmm_csr_rowgroup_rowmajor_bf16") == native
        torch.cuda.synchronize()


def test_value_refresh_and_capture(sx, oracle):
    """5. New values through update_values_device reach the native kernels (they read the arrays a refresh rewrites); after
    prepare_rm_bf16 a native call is captured into a graph and replayed with B rewritten in between."""
    import torch
    from sextans_amd import api
    rs = np.random.RandomState(21)
    M, K, N = 9000, 8000, 32
    rp, ci, v = random_csr(rs, M, K, 10, long_rows=2)
    v2 = rs.uniform(-1, 1, v.size).astype(np.float32)
    B16, B32, C32, C16 = operands(3, K, M, N)
    d_rp, d_ci = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda()
    d_v, d_v2 = torch.from_numpy(v).cuda(), torch.from_numpy(v2).cuda()
    st = torch.cuda.current_stream().cuda_stream
    with sx.Engine(0) as e, sx.Engine(0) as fresh:
        e.set_matrix_csr_device(M, K, v.size, d_rp.data_ptr(), d_ci.data_ptr(), d_v.data_ptr())
        check(e, B16, C32, _want(oracle, M, K, N, rp, ci, v, B32, C32), True)      # (plans and piece tables exist now)
        e.update_values_device(d_v2.data_ptr(), st)
        fresh.set_matrix_csr(M, K, rp, ci, v2)
        for cb in (False, True):
            C0, c32 = (C16, widen(C16)) if cb else (C32, C32)
            want = _want(oracle, M, K, N, rp, ci, v2, B32, c32)
            a = check(e, B16, C0, want, True)
            b = check(fresh, B16, C0, want, True)
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
            assert e.last_kernel() == fresh.last_kernel() and e.last_kernel().startswith("spmm_csr_rowgroup_rowmajor_bf16"), e.last_kernel()
    for cb in (False, True):
        with sx.Engine(0) as e:
            e.set_matrix_csr(M, K, rp, ci, v)
            e.prepare_rm_bf16(N, api.DTYPE_BF16 if cb else api.DTYPE_F32)
            build_s, held = e.get_stat("plan_build_s"), e.get_stat("device_bytes")
            dB = torch.zeros((K, N), dtype=torch.bfloat16, device="cuda")
            dCin = torch.from_numpy((C16 if cb else C32).view(np.int16) if cb else C32).cuda()
            dC = torch.zeros((M, N), dtype=torch.int16 if cb else torch.float32, device="cuda")
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                e.spmm_device_rm_bf16(N, float(ALPHA), dB.data_ptr(), N, float(BETA), dCin.data_ptr(), N, dC.data_ptr(), N,
                                      api.DTYPE_BF16 if cb else api.DTYPE_F32, torch.cuda.current_stream().cuda_stream)
            assert e.get_stat("plan_build_s") == build_s and e.get_stat("device_bytes") == held and counts(e) == (1, 0)
            for trial in range(3):
                Bt16 = to_bf16(np.random.RandomState(100 + trial).uniform(-1, 1, (K, N)))
                dB.view(torch.int16).copy_(torch.from_numpy(Bt16.view(np.int16)))
                g.replay()
                torch.cuda.synchronize()
                want = _want(oracle, M, K, N, rp, ci, v, widen(Bt16), widen(C16) if cb else C32)
                got = dC.cpu().numpy()
                assert same16(got.view(np.uint16), to_bf16(want)) if cb else bits_equal(got, want), (cb, trial)


def test_rounding_edge_values(sx, oracle):
    """6. fp32 -> bf16 of the result, element for element against torch's CPU rounding: ties (to even, both directions), +-0, +-inf,
    the largest finite fp32 (-> inf), subnormals, NaN (0 * inf) -- through the native kernel's epilogue and through the converter."""
    M = K = N = 64
    tie = np.float32(1.0 + 2.0 ** -8)          # a * b with b in bf16 lies exactly between two bf16 values
    tie_odd = np.float32(1.0 + 2.0 ** -7 + 2.0 ** -8)   # ... and this one between an odd bf16 below and an even one above
    a = np.array([tie, -tie, 1.0, np.finfo(np.float32).max, 2.0 ** -100, 1.0 - 2.0 ** -9, 0.5, tie_odd] * 8, np.float32)
    rp = np.arange(M + 1, dtype=np.int32); ci = np.arange(M, dtype=np.int32)
    rs = np.random.RandomState(6)
    B16 = rs.randint(0, 1 << 16, (K, N)).astype(np.uint16)             # random bit patterns ...
    exp = (B16 >> 7) & 0xff
    B16[exp == 0xff] &= 0xff80                                          # ... without NaNs of their own (payloads are not compared)
    B16[:, 0] = 0x0000; B16[:, 1] = 0x8000; B16[:, 2] = 0x7f80; B16[:, 3] = 0xff80      # +-0, +-inf
    B16[:, 4] = 0x0001; B16[:, 5] = 0x807f; B16[:, 6] = 0x3f80; B16[:, 7] = 0x3f81      # subnormals, 1.0 (even), 1.0078125 (odd)
    B16[:, 8] = 0x7f7f; B16[:, 9] = 0x0080                                              # largest finite bf16, smallest normal
    B32 = widen(B16)
    C16 = np.zeros((M, N), np.uint16)
    C16[5, :] = 0x7f80                                                  # beta * C_in = 0 * inf: a row of NaNs
    want = _want(oracle, M, K, N, rp, ci, a, B32, widen(C16), np.float32(1.0), np.float32(0.0))
    assert want[3, 6] == np.finfo(np.float32).max and np.all(np.isnan(want[5])) and want[0, 6] == tie and want[7, 6] == tie_odd
    for kernel in (0, 1):                          # the dispatcher's choice for a tiny matrix, and the gather kernel asked for
        with sx.Engine(0) as e:
            e.set_option("kernel", kernel)
            e.set_matrix_csr(M, K, rp, ci, a)
            native, got32 = rule(e, M, K, N, B32, widen(C16), True, alpha=1.0, beta=0.0)
            assert bits_equal(got32, want)
            got = check(e, B16, C16, want, native, alpha=1.0, beta=0.0)
            assert same16(got, to_bf16(want))
            if kernel == 1:
                assert native and e.last_kernel() == "spmm_csr_rowgroup_rowmajor_bf16", e.last_kernel()
    t = to_bf16(want)
    assert t[0, 6] == 0x3f80 and t[7, 6] == 0x3f82 and t[1, 6] == 0xbf80 and t[3, 6] == 0x7f80    # ties to even, down and up; FLT_MAX -> inf
