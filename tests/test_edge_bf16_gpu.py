"""bf16 edge tensors on the GPU through the C ABI (sextans_edge_op_device_rm_bf16 / _backward_device_rm_bf16,
sextans_spmm_edge_device_rm_bf16 / _backward_device_rm_bf16).  The contract under test: a bf16 value read is widened exactly, every
operation and sum is the fp32 entry point's, a bf16 value written is its fp32 result rounded once to nearest even.  So
  dealing    on the 92-row pattern P of test_pattern_dealing_gpu.py and its transpose, at every slot width plus N = 136, integer operands
             in [-4, 4]: every value is an integer of magnitude at most 20 (exact in bf16: 8 significant bits hold 256), every partial
             sum an exact fp32 integer, and Z, dE, C, dB, dx_dst, dx_src EQUAL the int64 computation;
  bits       on the 400 x 300 matrix of the reduce tests with bf16 edge tensors rounded from uniform fp32: every bf16 output is
             to_bf16(the fp32 entry point's output on the widened inputs), every fp32 output is bit-equal to that run -- all ops of both
             families, each gradient alone and together;
  and special values, padding, degenerate matrices and determinism (runs, streams, a captured graph replayed twice).
No tolerance anywhere: every comparison is on bits (bf16 NaNs compared as NaNs, as to_bf16's own test does).
Every bf16 tensor sits in a buffer with a padded leading dimension whose padding holds the pattern 0x5A5A: an input's padding that were
read would change a result, an output's padding must come back untouched."""
import numpy as np
import pytest

import test_edge_op_gpu as eop
import test_spmm_edge_gpu as sedge
from test_bf16_operands_gpu import same16, to_bf16, widen
from test_fused_attention_gpu import rand, same
from test_pattern_dealing_gpu import TILED, pat, rng
from test_spmm_edge_gpu import ints, rows_of
from test_spmm_reduce_gpu import POISON, base_matrix

pytestmark = pytest.mark.gpu

OPS = eop.OPS              # edge_op: add sub mul dst src
EOPS = sedge.OPS           # spmm_edge: mul add add_relu copy
GRADS = eop.GRADS
SIZES = eop.SIZES          # 8, 24, 72, 200: one tile; a partial tile; two tiles the last one partial; a tile of 128 and a partial one
POISON16 = POISON & 0xFFFF                      # 0x5A5A: a finite bf16 (about 1.5e13)
PAD_E, PAD_Z, PAD_G, PAD_DE = 4, 12, 8, 4       # extra columns of the bf16 buffers (leading dimensions: multiples of 4)


class Bf16Abi(eop.EdgeOpAbi):
    """one engine on a pattern: the four bf16 entry points, and their fp32 twins (eop.EdgeOpAbi.fwd / .bwd, sedge.Abi.forward / .backward)
    on the same engine"""
    buf = sedge.Abi.buf

    def dev16(self, b16, pad, rows=None):
        """(rows, N) uint16 bit patterns -> a (rows, N + pad) int16 device buffer whose padding holds POISON16, or None"""
        if b16 is None:
            return None
        tc = self.t
        out = tc.full((max(b16.shape[0], 1), b16.shape[1] + pad), POISON16, dtype=tc.int16, device="cuda")
        out[:b16.shape[0], :b16.shape[1]] = tc.from_numpy(np.ascontiguousarray(b16).view(np.int16))
        return out

    def out16(self, rows, N, pad):
        tc = self.t
        return tc.full((max(rows, 1), N + pad), POISON16, dtype=tc.int16, device="cuda")

    @staticmethod
    def host16(buf, rows):
        return buf.cpu().numpy().view(np.uint16)[:rows]

    def stream(self):
        return self.t.cuda.current_stream().cuda_stream

    # --- edge_op ---
    def fwd16(self, op, xd, xs, E16, N=None):
        """-> Z (nnz, N) uint16 and the whole padded buffer"""
        N = N or (xd if xd is not None else xs).shape[1]
        db, sb, Eb = self.dev(xd), self.dev(xs), self.dev16(E16, PAD_E)
        Zb = self.out16(self.nnz, N, PAD_Z)
        ptr = lambda x: x.data_ptr() if x is not None else None   # noqa: E731
        self.eng.edge_op_device_rm_bf16(OPS[op], N, ptr(db), N, ptr(sb), N, ptr(Eb), N + PAD_E, Zb.data_ptr(), N + PAD_Z, self.stream())
        self.t.cuda.synchronize()
        Zn = self.host16(Zb, self.nnz)
        return Zn[:, :N], Zn

    def bwd16(self, op, xd, xs, Gz16, want=GRADS):
        """-> {name: numpy fp32}; the gradient not in `want` gets no pointer and keeps its 7.0"""
        tc = self.t
        N = Gz16.shape[1]
        db, sb, Gb = self.dev(xd), self.dev(xs), self.dev16(Gz16, PAD_G)
        buf = {"dxdst": tc.full((max(self.M, 1), N), 7.0, device="cuda"), "dxsrc": tc.full((max(self.K, 1), N), 7.0, device="cuda")}
        p = {k: (x.data_ptr() if k in want else None) for k, x in buf.items()}
        ptr = lambda x: x.data_ptr() if x is not None else None   # noqa: E731
        self.eng.edge_op_backward_device_rm_bf16(OPS[op], N, ptr(db), N, ptr(sb), N, Gb.data_ptr(), N + PAD_G, p["dxdst"], N, p["dxsrc"], N,
                                                 self.stream())
        tc.cuda.synchronize()
        return {"dxdst": buf["dxdst"].cpu().numpy()[:self.M], "dxsrc": buf["dxsrc"].cpu().numpy()[:self.K]}

    # --- spmm_edge ---
    def sfwd16(self, op, B, E16):
        """-> C (M, N) fp32"""
        tc = self.t
        N = E16.shape[1]
        Bb = self.buf(B, 0) if op != "copy" else None
        Eb = self.dev16(E16, PAD_E)
        Cb = tc.full((max(self.M, 1), N), 7.0, device="cuda")
        self.eng.spmm_edge_device_rm_bf16(EOPS[op], N, Bb.data_ptr() if Bb is not None else None, N, Eb.data_ptr(), N + PAD_E, Cb.data_ptr(), N,
                                          self.stream())
        tc.cuda.synchronize()
        return Cb.cpu().numpy()[:self.M]

    def sbwd16(self, op, B, E16, G, want_dB=True, want_dE=True):
        """-> dB fp32 (None for copy / not asked for), dE uint16 (None when not asked for), dE's whole padded buffer"""
        tc = self.t
        N = G.shape[1]
        want_dB = want_dB and op != "copy"
        need_b = op == "add_relu" or (op == "mul" and want_dE)
        need_e = op == "add_relu" or (op == "mul" and want_dB)
        Bb = self.buf(B, 0) if need_b else None       # what the op's gradients do not read is passed as NULL
        Eb = self.dev16(E16, PAD_E) if need_e else None
        Gb = self.buf(G, 0)
        dB = tc.full((self.K, N), 7.0, device="cuda") if want_dB else None
        dE = self.out16(self.nnz, N, PAD_DE) if want_dE else None
        ptr = lambda x: x.data_ptr() if x is not None else None   # noqa: E731
        self.eng.spmm_edge_backward_device_rm_bf16(EOPS[op], N, ptr(Bb), N, ptr(Eb), N + PAD_E, Gb.data_ptr(), N, ptr(dB), N, ptr(dE),
                                                   N + PAD_DE, self.stream())
        tc.cuda.synchronize()
        dEn = self.host16(dE, self.nnz) if want_dE else None
        return (dB.cpu().numpy() if want_dB else None), (dEn[:, :N] if want_dE else None), dEn

    # --- the fp32 twins of spmm_edge on this engine ---
    def sfwd32(self, op, B, E):
        return sedge.Abi.forward(self, op, B, E)[0]

    def sbwd32(self, op, B, E, G, **kw):
        return sedge.Abi.backward(self, op, B, E, G, **kw)[:2]


def untouched(buf, N):
    """the padding columns of a bf16 output buffer"""
    return bool(np.all(buf[:, N:] == POISON16))


def i16(x):
    """an integer-valued array as bf16 bit patterns (exact: magnitudes at most 20)"""
    b = to_bf16(np.asarray(x, np.float32))
    assert np.array_equal(widen(b), np.asarray(x, np.float32))
    return b


# --- dealing: every path, every width, exact integers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["P", "PT"])
@pytest.mark.parametrize("N", TILED)
def test_every_dealing_path_exact_on_integers(sx, N, name):
    p, other = pat(name), pat("PT" if name == "P" else "P")   # other: the pattern the column passes walk
    assert p.long_rows != other.long_rows
    rs = rng("edge_bf16", N, name)
    xd, xs, E, Gz = ints(rs, p.M, N), ints(rs, p.K, N), ints(rs, p.nnz, N), ints(rs, p.nnz, N)
    G = ints(rs, p.M, N)
    E16, Gz16 = i16(E), i16(Gz)
    tag = lambda base, long: base + ("+long_rows" if long else "")   # noqa: E731
    a = Bf16Abi(sx, p.rp, p.ci, p.M, p.K)
    for op in OPS:
        for e, e16 in ((None, None), (E, E16)):
            Z, Zb = a.fwd16(op, xd, xs, e16)
            assert a.eng.last_kernel() == tag("edge_op_bf16", p.long_rows), (op, a.eng.last_kernel())
            want = eop.forward_ref(op, p.rp, p.ci, xd, xs, e, np.int64)
            assert np.abs(want).max() <= 20
            assert np.array_equal(widen(Z), want.astype(np.float32)) and untouched(Zb, N), (op, e is not None)
        names = eop.grads_of(op)
        got = a.bwd16(op, xd, xs, Gz16, want=names)
        long = ("dxdst" in names and p.long_rows) or ("dxsrc" in names and other.long_rows)
        assert a.eng.last_kernel() == tag("edge_op_backward_bf16", long), (op, a.eng.last_kernel())
        want, _, _ = eop.backward_ref(op, p.rp, p.ci, xd, xs, Gz, p.M, p.K, np.int64)
        for g in names:
            assert np.array_equal(got[g], want[g].astype(np.float32)), (op, g)
        if len(names) == 2:   # each pass alone names the kernel of the pattern it walks
            a.bwd16(op, xd, xs, Gz16, want=("dxdst",))
            assert a.eng.last_kernel() == tag("edge_op_backward_bf16", p.long_rows)
            a.bwd16(op, xd, xs, Gz16, want=("dxsrc",))
            assert a.eng.last_kernel() == tag("edge_op_backward_bf16", other.long_rows)
    for op in EOPS:
        wC, wdB, wdE, _, _ = sedge.reference(op, p.rp, p.ci, xs, E, G, p.K, dtype=np.int64)
        assert np.abs(wdE).max() <= 20
        C = a.sfwd16(op, xs, E16)
        assert a.eng.last_kernel() == tag("spmm_edge_bf16", p.long_rows), (op, a.eng.last_kernel())
        assert np.array_equal(C, wC.astype(np.float32)), op
        dB, dE, dEb = a.sbwd16(op, xs, E16, G)
        assert a.eng.last_kernel() == tag("spmm_edge_backward_bf16", True if op != "copy" else p.long_rows), (op, a.eng.last_kernel())
        assert np.array_equal(widen(dE), wdE.astype(np.float32)) and untouched(dEb, N), op
        if op == "copy":
            assert dB is None
            continue
        assert np.array_equal(dB, wdB.astype(np.float32)), op
        a.sbwd16(op, xs, E16, G, want_dE=False)
        assert a.eng.last_kernel() == tag("spmm_edge_backward_bf16", other.long_rows)
        a.sbwd16(op, xs, E16, G, want_dB=False)
        assert a.eng.last_kernel() == tag("spmm_edge_backward_bf16", p.long_rows)
    a.eng.close()


# --- bits on real operands -----------------------------------------------------------------------------------------------------------------
_cases = {}


def base_case(N):
    """the 400 x 300 matrix of the reduce tests (empty rows, one row of 300); node operands uniform in +-1, the edge tensors uniform fp32
    rounded to bf16; once per N, never changed"""
    if N not in _cases:
        rs, rp, ci, _, M, K = base_matrix(5)
        nnz = len(ci)
        _cases[N] = (rp, ci, M, K, rand(rs, M, N), rand(rs, K, N), to_bf16(rand(rs, nnz, N)), to_bf16(rand(rs, nnz, N)), rand(rs, M, N))
    return _cases[N]


@pytest.mark.parametrize("N", SIZES)
def test_edge_op_has_the_bits_of_the_fp32_entry_on_the_widened_inputs(sx, N):
    rp, ci, M, K, xd, xs, E16, Gz16, _ = base_case(N)
    E, Gz = widen(E16), widen(Gz16)
    a = Bf16Abi(sx, rp, ci, M, K)
    for op in OPS:
        for e, e16 in ((None, None), (E, E16)):
            Z16, Zb = a.fwd16(op, xd, xs, e16)
            assert a.eng.last_kernel() == "edge_op_bf16"
            Z32, _ = a.fwd(op, xd, xs, e)
            assert a.eng.last_kernel() == "edge_op"
            assert np.array_equal(Z16, to_bf16(Z32)) and untouched(Zb, N), (op, e is not None)
            if op in ("add", "sub", "mul") or e is not None:
                assert np.any(widen(Z16) != Z32)   # (the rounding is not vacuous)
        names = eop.grads_of(op)
        got = a.bwd16(op, xd, xs, Gz16, want=names)
        assert a.eng.last_kernel() == "edge_op_backward_bf16"
        ref = a.bwd(op, xd, xs, Gz, want=names)
        for g in GRADS:
            assert same(got[g], ref[g]), (op, g)       # (the one not asked for: 7.0 in both)
        for g in names:                                # each gradient alone: the same bits, the other's buffer untouched
            alone = a.bwd16(op, xd, xs, Gz16, want=(g,))
            assert same(alone[g], ref[g]) and np.all(alone[[x for x in GRADS if x != g][0]] == 7.0), (op, g)
    a.eng.close()


@pytest.mark.parametrize("N", SIZES)
def test_spmm_edge_has_the_bits_of_the_fp32_entry_on_the_widened_inputs(sx, N):
    rp, ci, M, K, _, B, E16, _, G = base_case(N)
    E = widen(E16)
    a = Bf16Abi(sx, rp, ci, M, K)
    for op in EOPS:
        C = a.sfwd16(op, B, E16)
        assert a.eng.last_kernel() == "spmm_edge_bf16"
        assert same(C, a.sfwd32(op, B, E)), op
        assert a.eng.last_kernel() == "spmm_edge"
        dB, dE16, dEb = a.sbwd16(op, B, E16, G)
        assert a.eng.last_kernel() == "spmm_edge_backward_bf16"
        rB, rE = a.sbwd32(op, B, E, G)
        assert np.array_equal(dE16, to_bf16(rE)) and untouched(dEb, N), op
        if op == "mul":
            assert np.any(widen(dE16) != rE)
        _, alone, _ = a.sbwd16(op, B, E16, G, want_dB=False)
        assert np.array_equal(alone, dE16), op
        if op == "copy":
            assert dB is None
            continue
        assert same(dB, rB), op
        assert same(a.sbwd16(op, B, E16, G, want_dE=False)[0], rB), op
    a.eng.close()


# --- special values --------------------------------------------------------------------------------------------------------------------------
NAN16, INF16, NINF16, NZERO16 = 0x7FC0, 0x7F80, 0xFF80, 0x8000
BIG = np.float32(2.0 ** 64)
EDGE = np.array([0x5F7FC000], np.uint32).view(np.float32)[0]   # BIG * EDGE = 0x7F7FC000: finite in fp32, above bf16's rounding boundary


def test_special_values(sx):
    """NaN, +-inf and -0 in E and Gz, and a product that overflows bf16 but not fp32: each shows in its own (entry, column), in the row
    and the column that hold it, and nowhere else, rounded as the contract says"""
    N = 24
    rp, ci, M, K, xd, xs, E16, Gz16, G = base_case(N)
    rows = rows_of(rp)
    nnz = len(ci)
    e1, e0 = nnz // 3, (2 * nnz) // 3                # the entry with E's special values, the one with Gz's
    eo = nnz // 2                                    # the entry whose product overflows bf16, at column 9
    ro, co = int(rows[eo]), int(ci[eo])
    assert len({int(rows[e]) for e in (e1, e0, eo)}) == 3 and len({int(ci[e]) for e in (e1, e0, eo)}) == 3
    E2, Gz2 = E16.copy(), Gz16.copy()
    E2[e1, [3, 17, 20, 6]] = NAN16, INF16, NINF16, NZERO16
    Gz2[e0, [5, 11, 2]] = NAN16, NINF16, NZERO16
    xd2, xs2 = xd.copy(), xs.copy()
    xd2[ro, 9], xs2[co, 9] = BIG, EDGE
    a = Bf16Abi(sx, rp, ci, M, K)
    # edge_op forward: E's values in their entry, the overflow in its entry
    for op in OPS:
        Z16, _ = a.fwd16(op, xd2, xs2, E2)
        Z32, _ = a.fwd(op, xd2, xs2, widen(E2))
        assert same16(Z16, to_bf16(Z32)), op
        hit = np.zeros(Z16.shape, bool)
        hit[e1, [3, 17, 20]] = True
        if op == "mul":
            hit[eo, 9] = True
            assert np.isfinite(Z32[eo, 9]) and Z16[eo, 9] == INF16
        assert np.array_equal(~np.isfinite(widen(Z16)), hit), op
        assert Z16[e1, 17] == INF16 and Z16[e1, 20] == NINF16 and np.isnan(widen(Z16[e1, 3:4]))[0]
    Z16, _ = a.fwd16("dst", -np.zeros_like(xd), None, None, N=N)   # -0 stays -0
    assert np.all(Z16 == NZERO16)
    # edge_op backward: Gz's values in the row and the column of their entry
    for op in OPS:
        names = eop.grads_of(op)
        got, ref = a.bwd16(op, xd, xs, Gz2, want=names), a.bwd(op, xd, xs, widen(Gz2), want=names)
        for g in names:
            hit = np.zeros(got[g].shape, bool)
            hit[rows[e0] if g == "dxdst" else ci[e0], [5, 11]] = True
            assert np.array_equal(~np.isfinite(got[g]), hit), (op, g)
            assert same(got[g][~hit], ref[g][~hit]) and np.array_equal(np.isnan(got[g]), np.isnan(ref[g])), (op, g)
    # spmm_edge: E's values reach C's row and dB's column of their entry; dE = G * B overflows in its entry
    G2, B2 = G.copy(), xs.copy()
    G2[ro, 9], B2[co, 9] = BIG, EDGE
    for op in EOPS:
        C, rC = a.sfwd16(op, xs, E2), a.sfwd32(op, xs, widen(E2))
        hit = np.zeros(C.shape, bool)
        hit[rows[e1], [3, 17] + ([] if op == "add_relu" else [20])] = True   # (relu(-inf) = 0)
        assert np.array_equal(~np.isfinite(C), hit), op
        assert same(C[~hit], rC[~hit]) and np.array_equal(np.isnan(C), np.isnan(rC)), op
        dB, dE16, _ = a.sbwd16(op, B2, E2, G2)
        rB, rE = a.sbwd32(op, B2, widen(E2), G2)
        assert same16(dE16, to_bf16(rE)), op
        if op == "mul":
            assert np.isfinite(rE[eo, 9]) and dE16[eo, 9] == INF16
            hit = np.zeros(dE16.shape, bool)
            hit[eo, 9] = True
            assert np.array_equal(~np.isfinite(widen(dE16)), hit)
        if op != "copy":
            assert np.array_equal(np.isnan(dB), np.isnan(rB)) and same(dB[~np.isnan(dB)], rB[~np.isnan(rB)]), op
            bad = np.flatnonzero(~np.isfinite(dB).all(axis=1))
            assert set(bad) <= {int(ci[e1]), co}, op   # only the columns of the two entries
    G3 = G.copy()
    G3[rows[e1], 6] = -0.0
    _, dE16, _ = a.sbwd16("copy", None, E2, G3)        # dE = G[r]: -0 stays -0
    assert dE16[e1, 6] == NZERO16
    a.eng.close()


# --- degenerate matrices -------------------------------------------------------------------------------------------------------------------
def test_degenerate_matrices(sx):
    """no rows, and no entries: OK, Z and dE have no element, C, dB, dx_dst and dx_src are zeroed, last_kernel stays what it was"""
    N = 16
    rs = np.random.RandomState(4)
    for M, K in ((0, 7), (9, 7)):
        rp, ci = np.zeros(M + 1, np.int32), np.zeros(0, np.int32)
        xd, xs, G, none16 = rand(rs, M, N), rand(rs, K, N), rand(rs, M, N), np.zeros((0, N), np.uint16)
        a = Bf16Abi(sx, rp, ci, M, K)
        before = a.eng.last_kernel()
        for op in OPS:
            Z, Zb = a.fwd16(op, xd, xs, none16)
            assert Z.shape == (0, N)
            got = a.bwd16(op, xd, xs, none16, want=eop.grads_of(op))
            for g in eop.grads_of(op):
                assert got[g].shape == ((M if g == "dxdst" else K), N) and np.all(got[g].view(np.uint32) == 0), (op, g)
        for op in EOPS:
            C = a.sfwd16(op, xs, none16)
            assert C.shape == (M, N) and np.all(C.view(np.uint32) == 0), op
            dB, dE, dEb = a.sbwd16(op, xs, none16, G)
            assert dE.shape == (0, N)
            if op != "copy":
                assert dB.shape == (K, N) and np.all(dB.view(np.uint32) == 0), op
        assert a.eng.last_kernel() == before
        a.eng.close()


# --- determinism -----------------------------------------------------------------------------------------------------------------------------
def test_determinism_streams_and_graph_replay(sx):
    import torch
    N, op, sop = 24, "mul", "mul"
    rp, ci, M, K, xd, xs, E16, Gz16, G = base_case(N)
    a = Bf16Abi(sx, rp, ci, M, K)

    def all_four():
        Z, _ = a.fwd16(op, xd, xs, E16)
        g = a.bwd16(op, xd, xs, Gz16)
        C = a.sfwd16(sop, xs, E16)
        dB, dE, _ = a.sbwd16(sop, xs, E16, G)
        return [Z, g["dxdst"], g["dxsrc"], C, dB, dE]

    def eq(x, y):
        return np.array_equal(x, y) if x.dtype == np.uint16 else same(x, y)

    first, second = all_four(), all_four()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = all_four()
    torch.cuda.current_stream().wait_stream(side)
    for i, (x, y, z) in enumerate(zip(first, second, third)):
        assert eq(x, y) and eq(x, z), i

    # a fresh engine: prepare() alone builds the tables and A^T, then both families' forward and backward are captured on a single stream
    # and replayed twice
    b = Bf16Abi(sx, rp, ci, M, K)
    b.eng.prepare(N, True, torch.cuda.current_stream().cuda_stream, transposed=True)
    torch.cuda.synchronize()
    dt, st, Gt = b.dev(xd), b.dev(xs), b.buf(G, 0)
    Et, Gzt = b.dev16(E16, PAD_E), b.dev16(Gz16, PAD_G)
    Zt, dEt = b.out16(b.nnz, N, PAD_Z), b.out16(b.nnz, N, PAD_DE)
    dd, ds, Ct, dBt = (torch.zeros((r, N), device="cuda") for r in (M, K, M, K))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        s = torch.cuda.current_stream().cuda_stream
        b.eng.edge_op_device_rm_bf16(OPS[op], N, dt.data_ptr(), N, st.data_ptr(), N, Et.data_ptr(), N + PAD_E, Zt.data_ptr(), N + PAD_Z, s)
        b.eng.edge_op_backward_device_rm_bf16(OPS[op], N, dt.data_ptr(), N, st.data_ptr(), N, Gzt.data_ptr(), N + PAD_G, dd.data_ptr(), N,
                                              ds.data_ptr(), N, s)
        b.eng.spmm_edge_device_rm_bf16(EOPS[sop], N, st.data_ptr(), N, Et.data_ptr(), N + PAD_E, Ct.data_ptr(), N, s)
        b.eng.spmm_edge_backward_device_rm_bf16(EOPS[sop], N, st.data_ptr(), N, Et.data_ptr(), N + PAD_E, Gt.data_ptr(), N, dBt.data_ptr(), N,
                                                dEt.data_ptr(), N + PAD_DE, s)
    for _ in range(2):
        for t in (Zt, dd, ds, Ct, dBt, dEt):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = [b.host16(Zt, b.nnz)[:, :N], dd.cpu().numpy(), ds.cpu().numpy(), Ct.cpu().numpy(), dBt.cpu().numpy(), b.host16(dEt, b.nnz)[:, :N]]
        for i, (x, y) in enumerate(zip(got, first)):
            assert eq(x, y), i
    a.eng.close()
    b.eng.close()
