"""bf16 edge tensors of the gated aggregation on the GPU through the C ABI (sextans_spmm_gated_device_rm_bf16 /
sextans_spmm_gated_backward_device_rm_bf16).  The contract under test: a bf16 value read (E, Gz) is widened exactly, every operation
and every sum is the fp32 entry point's, in its order; a bf16 value written (z, dE) is its fp32 result rounded once to nearest even, and
the rounded value never feeds back (the gate comes from the unrounded z_e, dxdst and dxsrc sum the unrounded dz_e).  So the reference of
every comparison is the fp32 entry point ON THE SAME ENGINE on the widened inputs -- tests/test_spmm_gated_gpu.py pins that one to
float64 -- and every comparison is on bits:
  fp32 outputs (C, den, dxdst, dxsrc, dV)   the twin's bits (same);
  bf16 outputs (z, dE)                      to_bf16(the twin's output) (bf16 NaNs compared as NaNs where special values are planted).
No tolerance anywhere.
  dealing    the 92-row pattern P of test_pattern_dealing_gpu.py and its transpose at N = 8, 16, 32, 64 (one width per slot shape): the
             full GatedGCN call; and the sharper check with integers that name their (entry, tile piece): z == E and dE == Gz;
  bits       the 400 x 300 matrix of the reduce tests at N = 8, 24, 72 (one tile; a partial tile; two tiles, the last one partial);
  and long rows, special values, degenerate matrices and determinism (runs, streams, a graph captured on a fresh prepared engine).
Every bf16 tensor sits in a buffer with a padded leading dimension whose padding holds the pattern 0x5A5A (the scheme of
test_edge_bf16_gpu.py): an input's padding that were read would change a result, an output's padding must come back untouched."""
import numpy as np
import pytest

from test_bf16_operands_gpu import same16, to_bf16, widen
from test_edge_bf16_gpu import POISON16, Bf16Abi, untouched
from test_fused_attention_gpu import edge_pattern, rand, same
from test_pattern_dealing_gpu import names_ok, pat, rng
from test_spmm_gated_gpu import GRADS, OUT, GatedAbi, base_case
from test_spmm_reduce_gpu import POISON
from test_spmm_softagg_gpu import cut_rows

pytestmark = pytest.mark.gpu

SUM, NORM = 1, 2
EPS = 1e-6
PAD_E, PAD_Z, PAD_GZ, PAD_DE = 4, 12, 8, 4   # extra columns of the bf16 buffers (leading dimensions: multiples of 4); E != z, Gz != dE
NAN16, INF16, NINF16, NZERO16 = 0x7FC0, 0x7F80, 0xFF80, 0x8000
BIG_Z = np.array([0x7F7FC000], np.uint32).view(np.float32)[0]   # finite in fp32, above bf16's rounding boundary 0x7F7F8000


class GatedBf16Abi(GatedAbi):
    """one engine on a pattern: the two bf16 entry points, and their fp32 twins (GatedAbi.fwd / .bwd) on the same engine"""
    dev16, out16, host16 = Bf16Abi.dev16, Bf16Abi.out16, staticmethod(Bf16Abi.host16)

    def stream(self):
        return self.t.cuda.current_stream().cuda_stream

    def operands16(self, xd, xs, V, E16):
        """-> (GatedIn whose d_e addresses bf16 at the leading dimension N + PAD_E, what it points to)"""
        gin, keep = self.operands(xd, xs, V, None)
        Eb = self.dev16(E16, PAD_E)
        if Eb is not None:
            gin.d_e, gin.ld_e = Eb.data_ptr(), E16.shape[1] + PAD_E
        return gin, keep + [Eb]

    def fwd16(self, mode, xd, xs, V, E16, want=OUT, eps=EPS):
        """-> {C, den: fp32; z: uint16 (nnz, N); z_buf: its whole padded buffer}; an output not in `want` gets no pointer and keeps its
        sentinel (POISON in C and den, as in GatedAbi.fwd; POISON16 in z)"""
        tc = self.t
        N = xd.shape[1]
        gin, keep = self.operands16(xd, xs, V, E16)
        Cb, Db = (tc.full((self.M, N), POISON, dtype=tc.int32, device="cuda") for _ in range(2))
        zb = self.out16(self.nnz, N, PAD_Z)
        p = {k: (x.data_ptr() if k in want else None) for k, x in (("C", Cb), ("den", Db), ("z", zb))}
        self.eng.spmm_gated_device_rm_bf16(mode, eps, N, gin, p["C"], N, p["den"], N, p["z"], N + PAD_Z, self.stream())
        tc.cuda.synchronize()
        zn = self.host16(zb, self.nnz)
        return {"C": Cb.cpu().numpy().view(np.float32), "den": Db.cpu().numpy().view(np.float32), "z": zn[:, :N], "z_buf": zn}

    def bwd16(self, mode, xd, xs, V, E16, f, G, Gz16=None, want=GRADS, eps=EPS):
        """-> {dxdst, dxsrc, dv: fp32; de: uint16 (nnz, N); de_buf: its whole padded buffer}; a gradient not in `want` gets no pointer and
        keeps its sentinel (7.0 / POISON16); f: the forward's C and den; the workspace is the twin's"""
        tc = self.t
        N = G.shape[1]
        gin, keep = self.operands16(xd, xs, V, E16)
        Ct, Dt, Gt = (tc.from_numpy(np.ascontiguousarray(x)).cuda() for x in (f["C"], f["den"], G))
        Gzb = self.dev16(Gz16, PAD_GZ)
        nwork = self.eng.spmm_gated_workspace_floats(mode, N)
        work = tc.full((max(nwork, 4),), 7.0, device="cuda")
        rows = {"dxdst": self.M, "dxsrc": self.K, "dv": self.K}
        buf = {k: tc.full((rows[k], N), 7.0, device="cuda") for k in rows}
        buf["de"] = self.out16(self.nnz, N, PAD_DE)
        out = self.sx.api.GatedGrad()
        for k in GRADS:
            if k in want:
                setattr(out, "d_" + k, buf[k].data_ptr())
            setattr(out, "ld_" + k, N + PAD_DE if k == "de" else N)
        self.eng.spmm_gated_backward_device_rm_bf16(mode, eps, N, gin, Ct.data_ptr(), N, Dt.data_ptr(), N, Gt.data_ptr(), N,
                                                    Gzb.data_ptr() if Gzb is not None else None, N + PAD_GZ, out,
                                                    work.data_ptr() if nwork else None, self.stream())
        tc.cuda.synchronize()
        res = {k: buf[k].cpu().numpy() for k in rows}
        res["de_buf"] = self.host16(buf["de"], self.nnz)
        res["de"] = res["de_buf"][:, :N]
        return res

    def fwd32(self, mode, xd, xs, V, E16, want=OUT, eps=EPS):
        return GatedAbi.fwd(self, mode, xd, xs, V, widen(E16) if E16 is not None else None, want=want, eps=eps)

    def bwd32(self, mode, xd, xs, V, E16, f, G, Gz16=None, want=GRADS, eps=EPS):
        return GatedAbi.bwd(self, mode, xd, xs, V, widen(E16) if E16 is not None else None, f, G,
                            widen(Gz16) if Gz16 is not None else None, want=want, eps=eps)


def same_nan(a, b):
    """fp32 bits; NaNs compared as NaNs (special values only)"""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and same(a[~na], b[~nb])


def matches(a, mode, xd, xs, V, E16, G, Gz16, fwant=OUT, gwant=GRADS, nan=False):
    """forward and backward on both entry points: fp32 outputs the twin's bits, bf16 outputs its outputs rounded, paddings untouched;
    what is not asked for keeps its sentinel.  -> (the bf16 run's forward, its gradients, the twin's forward, the twin's gradients, the
    two last_kernels of the bf16 run)"""
    N = xd.shape[1]
    eq16, eq32 = (same16, same_nan) if nan else (np.array_equal, same)
    f = a.fwd16(mode, xd, xs, V, E16, want=fwant)
    fwd = a.eng.last_kernel()
    r = a.fwd32(mode, xd, xs, V, E16, want=fwant)
    assert a.eng.last_kernel() == fwd.replace("_bf16", "")
    for k in ("C", "den"):
        assert eq32(f[k], r[k]), (mode, k)                       # (not asked for: POISON in both)
        assert (k in fwant) != bool(np.all(f[k].view(np.int32) == POISON)), (mode, k)
    if "z" in fwant:
        assert eq16(f["z"], to_bf16(r["z"])) and untouched(f["z_buf"], N), mode
    else:
        assert np.all(f["z_buf"] == POISON16) and np.all(r["z_buf"] == POISON), mode
    full = f if "den" in fwant else a.fwd16(mode, xd, xs, V, E16)   # (the backward reads C and den)
    got = a.bwd16(mode, xd, xs, V, E16, full, G, Gz16, want=gwant)
    bwd = a.eng.last_kernel()
    ref = a.bwd32(mode, xd, xs, V, E16, full, G, Gz16, want=gwant)
    assert a.eng.last_kernel() == bwd.replace("_bf16", "")
    for k in GRADS[:3]:
        assert eq32(got[k], ref[k]), (mode, k)                   # (not asked for: 7.0 in both)
        assert (k in gwant) != bool(np.all(got[k] == 7.0)), (mode, k)
    if "de" in gwant:
        assert eq16(got["de"], to_bf16(ref["de"])) and untouched(got["de_buf"], N), mode
    else:
        assert np.all(got["de_buf"] == POISON16) and np.all(ref["de_buf"] == 7.0), mode
    return f, got, r, ref, (fwd, bwd)


def bf16_names(names):
    """the twins' names_ok on the bf16 names with the suffix taken out: _bf16 sits between the family's name and +long_rows"""
    for n in names:
        assert "_bf16" in n and (n.endswith("_bf16") or n.endswith("_bf16+long_rows")), n
    return [n.replace("_bf16", "") for n in names]


# --- dealing: every path, one width per slot shape -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["P", "PT"])
@pytest.mark.parametrize("N", [8, 16, 32, 64])
def test_every_dealing_path(sx, N, name):
    """GatedGCN's full call (NORM, E, den, z, Gz, all four gradients) with the operands of test_spmm_gated_gpu.test_row_dealing, the
    edge tensors rounded to bf16; at N = 16 also SUM without E and a bf16 z"""
    p, rs = pat(name), rng("gated", N, name)
    xd, xs, V, G = rand(rs, p.M, N), rand(rs, p.K, N), rand(rs, p.K, N), rand(rs, p.M, N)
    E16, Gz16 = to_bf16(rand(rs, p.nnz, N)), to_bf16(rand(rs, p.nnz, N))
    a = GatedBf16Abi(sx, p.rp, p.ci, p.M, p.K)
    f, got, r, ref, kernels = matches(a, NORM, xd, xs, V, E16, G, Gz16)
    names_ok(p, "spmm_gated", *bf16_names(kernels))
    assert np.any(widen(f["z"]) != r["z"]) and np.any(widen(got["de"]) != ref["de"])          # (the rounding is not vacuous)
    assert np.all(f["C"][p.empty].view(np.uint32) == 0) and np.all(f["den"][p.empty].view(np.uint32) == 0)
    if N == 16:
        f, got, r, ref, kernels = matches(a, SUM, xd, xs, V, None, G, Gz16)                   # d_e == NULL: z without E, rounded
        names_ok(p, "spmm_gated", *bf16_names(kernels))
        assert np.any(widen(f["z"]) != r["z"])
    a.eng.close()


@pytest.mark.parametrize("name", ["P", "PT"])
def test_every_piece_comes_from_and_goes_to_its_own_slot(sx, name):
    """The twin comparison shares the loaders' indexing, so: xdst = xsrc = 0 and E[e, n] a small integer that names (e mod 64, n mod 4)
    and the piece n // 4 -- exact in bf16 -- must come back as z, bit for bit; with V = 0 and G = 0 the gate's share of dz is +0 and
    dE must be Gz, bit for bit.  A piece read from or stored to another entry's or another piece's slot would show."""
    N = 16
    p = pat(name)
    e, n = np.meshgrid(np.arange(p.nnz), np.arange(N), indexing="ij")
    code = ((e % 64) * 4 + n % 4 + 1).astype(np.float32)                 # 1 .. 256: 8 significant bits at most
    E = code * np.where((n // 4) % 2 == 0, 1.0, -1.0).astype(np.float32)    # the piece's parity in the sign
    Gz = -(257.0 - code) * np.where((n // 4) < 2, 1.0, -1.0).astype(np.float32)
    E16, Gz16 = to_bf16(E), to_bf16(Gz)
    assert np.array_equal(widen(E16), E) and np.array_equal(widen(Gz16), Gz)
    zd, zs = np.zeros((p.M, N), np.float32), np.zeros((p.K, N), np.float32)
    a = GatedBf16Abi(sx, p.rp, p.ci, p.M, p.K)
    f = a.fwd16(NORM, zd, zs, zs, E16)
    fwd = a.eng.last_kernel()
    assert np.array_equal(f["z"], E16) and untouched(f["z_buf"], N)
    assert np.all(f["C"] == 0)                                           # V = 0
    g = a.bwd16(NORM, zd, zs, zs, E16, f, np.zeros((p.M, N), np.float32), Gz16)
    names_ok(p, "spmm_gated", *bf16_names((fwd, a.eng.last_kernel())))
    assert np.array_equal(g["de"], Gz16) and untouched(g["de_buf"], N)
    a.eng.close()


# --- bits on the 400 x 300 matrix ---------------------------------------------------------------------------------------------------------
_cases = {}


def case16(N, mode, with_e):
    """test_spmm_gated_gpu.base_case's operands, E and Gz rounded to bf16; once per case, never changed"""
    key = (N, mode, with_e)
    if key not in _cases:
        rp, ci, M, K, xd, xs, V, E, G, Gz, _ = base_case(N, mode, with_e)
        _cases[key] = (rp, ci, M, K, xd, xs, V, to_bf16(E) if with_e else None, G, to_bf16(Gz))
    return _cases[key]


@pytest.mark.parametrize("with_e", [False, True])
@pytest.mark.parametrize("mode", [SUM, NORM])
@pytest.mark.parametrize("N", [8, 24, 72])
def test_bits_of_the_fp32_entry_on_the_widened_inputs(sx, N, mode, with_e):
    rp, ci, M, K, xd, xs, V, E16, G, Gz16 = case16(N, mode, with_e)
    a = GatedBf16Abi(sx, rp, ci, M, K)
    f, got, r, ref, kernels = matches(a, mode, xd, xs, V, E16, G, Gz16)
    assert kernels == ("spmm_gated_bf16", "spmm_gated_backward_bf16")
    assert np.any(widen(f["z"]) != r["z"]) and np.any(widen(got["de"]) != ref["de"])
    # the forward without den and / or z: the same C, the others keep their sentinels
    for fwant in (("C",), ("C", "den"), ("C", "z")):
        f2 = matches(a, mode, xd, xs, V, E16, G, Gz16, fwant=fwant, gwant=("dxdst",))[0]
        assert same(f2["C"], f["C"]), fwant
    # each gradient alone: the same bits, the others' buffers untouched; then without Gz
    for k in GRADS:
        alone = matches(a, mode, xd, xs, V, E16, G, Gz16, fwant=("C", "den"), gwant=(k,))[1]
        assert np.array_equal(alone[k], got[k]) if k == "de" else same(alone[k], got[k]), k
    nogz = matches(a, mode, xd, xs, V, E16, G, None, fwant=("C", "den"))[1]
    assert not np.array_equal(nogz["de"], got["de"])
    a.eng.close()


# --- long rows ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [SUM, NORM])
def test_long_rows(sx, mode):
    """rows of 1 .. 300 entries, one of 2500 (the workgroup path) and a column of more than 2048 entries (the column pass's)"""
    rs = np.random.RandomState(8)
    rp, ci, _, M, K = edge_pattern(rs)
    assert np.count_nonzero(ci == 0) > 2048 and np.diff(rp).max() == 2500
    N, nnz = 24, len(ci)
    xd, xs, V, G = rand(rs, M, N), rand(rs, K, N), rand(rs, K, N), rand(rs, M, N)
    E16, Gz16 = to_bf16(rand(rs, nnz, N)), to_bf16(rand(rs, nnz, N))
    a = GatedBf16Abi(sx, rp, ci, M, K)
    _, _, _, _, kernels = matches(a, mode, xd, xs, V, E16, G, Gz16)
    assert kernels == ("spmm_gated_bf16+long_rows", "spmm_gated_backward_bf16+long_rows")
    a.eng.close()


# --- special values ---------------------------------------------------------------------------------------------------------------------------
def small_case():
    """a handful of rows at N = 8: lengths 3, 1, 0, 4, 2, 1 over 7 columns"""
    cols = [[0, 2, 5], [3], [], [1, 2, 4, 6], [0, 6], [5]]
    rs = np.random.RandomState(29)
    M, K, N = len(cols), 7, 8
    rp = np.zeros(M + 1, np.int32); rp[1:] = np.cumsum([len(c) for c in cols])
    ci = np.array(sum(cols, []), np.int32)
    nnz = len(ci)
    return (rp, ci, M, K, N, rand(rs, M, N), rand(rs, K, N), rand(rs, K, N), to_bf16(rand(rs, nnz, N)), rand(rs, M, N),
            to_bf16(rand(rs, nnz, N)))


def quiet(b16):
    """every NaN among these bf16 patterns is a quiet one"""
    nan = np.isnan(widen(b16))
    return bool(np.all(b16[nan] & 0x40))


@pytest.mark.parametrize("mode", [SUM, NORM])
def test_special_values_stay_in_their_entry_row_and_column(sx, mode):
    """a bf16 NaN, +-inf and -0 in E and in Gz: each shows in its own (entry, column) of z / dE, in the (row, column) of C, den and dxdst
    and the (column, column) of dxsrc and dV that hold it, and nowhere else -- exactly as in the twin; a bf16 NaN written is a quiet one"""
    rp, ci, M, K, N, xd, xs, V, E16, G, Gz16 = small_case()
    rows = np.repeat(np.arange(M), np.diff(rp))
    e1, e0 = 1, 8                                    # the entry with E's special values (row 0, column 2), the one with Gz's (row 4, column 0)
    assert rows[e1] == 0 and ci[e1] == 2 and rows[e0] == 4 and ci[e0] == 0
    E2, Gz2 = E16.copy(), Gz16.copy()
    E2[e1, [3, 5, 6, 1]] = NAN16, INF16, NINF16, NZERO16
    a = GatedBf16Abi(sx, rp, ci, M, K)
    f, got, r, ref, _ = matches(a, mode, xd, xs, V, E2, G, Gz16, nan=True)
    hit = np.zeros(f["z"].shape, bool)
    hit[e1, [3, 5, 6]] = True
    assert np.array_equal(~np.isfinite(widen(f["z"])), hit) and quiet(f["z"])
    assert f["z"][e1, 5] == INF16 and f["z"][e1, 6] == NINF16 and np.isnan(widen(f["z"][e1, 3:4]))[0]
    assert f["z"][e1, 1] == to_bf16(r["z"])[e1, 1]                                   # (-0 in E: an ordinary sum)
    allowed = np.zeros((M, N), bool)
    allowed[0, [3, 5, 6]] = True                     # the entry's row and columns, nowhere else; the NaN is there
    for k in ("C", "den"):
        assert np.isnan(f[k][0, 3]) and not (~np.isfinite(f[k]) & ~allowed).any(), k
    assert quiet(got["de"]) and np.isnan(widen(got["de"][e1, 3:4]))[0]
    assert not np.delete(~np.isfinite(widen(got["de"])), np.arange(rp[0], rp[1]), axis=0).any()     # NORM: C's NaN reaches the row's entries
    assert not np.delete(~np.isfinite(got["dxdst"]), 0, axis=0).any()
    for k in ("dxsrc", "dv"):                        # only the columns of that row's entries
        assert set(np.flatnonzero(~np.isfinite(got[k]).all(axis=1))) <= set(ci[rp[0]:rp[1]].tolist()), k
    # Gz's special values: dE's own (entry, column), dxdst's row, dxsrc's column; dV does not read Gz
    Gz2[e0, [2, 4, 7]] = NAN16, NINF16, NZERO16
    f, got, r, ref, _ = matches(a, mode, xd, xs, V, E16, G, Gz2, nan=True)
    hit = np.zeros(got["de"].shape, bool)
    hit[e0, [2, 4]] = True
    assert np.array_equal(~np.isfinite(widen(got["de"])), hit) and quiet(got["de"]) and got["de"][e0, 4] == NINF16
    for k, where in (("dxdst", 4), ("dxsrc", int(ci[e0]))):
        bad = np.zeros(got[k].shape, bool)
        bad[where, [2, 4]] = True
        assert np.array_equal(~np.isfinite(got[k]), bad), k
    assert np.all(np.isfinite(got["dv"]))
    # -0 stays -0 through a write: gates of exactly +0, G = +0 and V < 0 make the gate's share fma(-0, +0, .), and Gz = -0 on an entry
    # gives dz = -0 there
    cold = np.full_like(xd, -200.0)
    Gz3 = Gz16.copy()
    Gz3[e0] = NZERO16
    f, got, _, _, _ = matches(a, mode, cold, xs, -np.abs(V), E16, np.zeros_like(G), Gz3)
    assert np.all(V != 0) and np.all(got["de"][e0] == NZERO16)
    a.eng.close()


@pytest.mark.parametrize("mode", [SUM, NORM])
def test_a_z_above_bf16_range_is_stored_as_inf(sx, mode):
    """xdst[r, n] = 0x7F7FC000 against an xsrc and an E of 0 there: z is finite in fp32 and at or above bf16's rounding boundary -- inf in
    the stored z, in the entries of row r at column n and only there, while the gate (exactly 1) comes from the fp32 z: C, den and the
    gradients have the twin's bits"""
    rp, ci, M, K, N, xd, xs, V, E16, G, Gz16 = small_case()
    r0, n0 = 3, 5
    xd2, xs2, E2 = xd.copy(), xs.copy(), E16.copy()
    xd2[r0, n0], xs2[:, n0], E2[:, n0] = BIG_Z, 0.0, 0
    a = GatedBf16Abi(sx, rp, ci, M, K)
    f, got, r, ref, _ = matches(a, mode, xd2, xs2, V, E2, G, Gz16)
    hit = np.zeros(f["z"].shape, bool)
    hit[rp[r0]:rp[r0 + 1], n0] = True
    assert np.all(r["z"][hit] == BIG_Z) and np.all(f["z"][hit] == INF16)
    assert np.array_equal(~np.isfinite(widen(f["z"])), hit)
    assert all(np.all(np.isfinite(f[k])) for k in ("C", "den")) and f["den"][r0, n0] == rp[r0 + 1] - rp[r0]
    a.eng.close()


@pytest.mark.parametrize("with_e", [False, True])
@pytest.mark.parametrize("mode", [SUM, NORM])
def test_saturated_gates(sx, mode, with_e):
    """test_spmm_gated_gpu.test_saturated_gates on the bf16 entry points: xdst = +200 -- every gate exactly 1, den the row length;
    xdst = -200 -- every gate exactly +0, C and den +0, and dE == Gz bit for bit"""
    N = 24
    rp0, ci0, M, K, xd, xs, V, E0, G, Gz0 = case16(N, mode, True)
    rp, ci, keep = cut_rows(rp0, ci0, np.arange(len(ci0), dtype=np.float32))
    keep = keep.astype(np.int64)
    E16, Gz16 = (E0[keep] if with_e else None), Gz0[keep]
    lens = np.diff(rp)
    a = GatedBf16Abi(sx, rp, ci, M, K)
    f, got, _, _, _ = matches(a, mode, np.full_like(xd, 200.0), xs, V, E16, G, None)
    assert np.array_equal(f["den"], np.repeat(lens[:, None], N, 1).astype(np.float32))
    assert np.all(got["de"] & 0x7FFF == 0)
    f, got, _, _, _ = matches(a, mode, np.full_like(xd, -200.0), xs, V, E16, G, Gz16)
    assert np.all(f["C"] == 0) and np.all(f["den"] == 0)
    assert np.array_equal(got["de"], Gz16) and np.all(got["dv"] == 0)
    a.eng.close()


# --- degenerate matrices -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [SUM, NORM])
def test_degenerate_matrices(sx, mode):
    """no entry at all: C, den, dxdst, dxsrc and dV are zero-filled, z and dE have no element and their buffers (the padding too) are
    left alone; no row at all"""
    rs = np.random.RandomState(3)
    M, K, N = 5, 6, 16
    xd, xs, V, G = rand(rs, M, N), rand(rs, K, N), rand(rs, K, N), rand(rs, M, N)
    none16 = np.zeros((0, N), np.uint16)
    zeros = lambda x, shape: x.shape == shape and np.all(np.ascontiguousarray(x).view(np.uint32) == 0)   # noqa: E731
    a = GatedBf16Abi(sx, np.zeros(M + 1, np.int32), np.zeros(0, np.int32), M, K)
    before = a.eng.last_kernel()
    f = a.fwd16(mode, xd, xs, V, none16)
    assert zeros(f["C"], (M, N)) and zeros(f["den"], (M, N)) and f["z"].shape == (0, N)
    g = a.bwd16(mode, xd, xs, V, none16, f, G, none16)
    assert zeros(g["dxdst"], (M, N)) and zeros(g["dxsrc"], (K, N)) and zeros(g["dv"], (K, N)) and g["de"].shape == (0, N)
    assert a.eng.last_kernel() == before
    a.eng.close()
    z = GatedBf16Abi(sx, np.zeros(1, np.int32), np.zeros(0, np.int32), 0, K)
    f = z.fwd16(mode, np.zeros((0, N), np.float32), xs, V, None)
    assert f["C"].shape == (0, N)
    g = z.bwd16(mode, np.zeros((0, N), np.float32), xs, V, None, f, np.zeros((0, N), np.float32))
    assert g["dxdst"].shape == (0, N) and zeros(g["dxsrc"], (K, N)) and zeros(g["dv"], (K, N))
    z.eng.close()


def test_degenerate_matrices_leave_the_padding_alone(sx):
    """no entry: the fills of C, den and the node gradients write N columns of a wider buffer and nothing else"""
    import torch
    rs = np.random.RandomState(5)
    M, K, N, pad = 5, 6, 16, 4
    xd, xs, V, G = rand(rs, M, N), rand(rs, K, N), rand(rs, K, N), rand(rs, M, N)
    a = GatedBf16Abi(sx, np.zeros(M + 1, np.int32), np.zeros(0, np.int32), M, K)
    gin, keep = a.operands16(xd, xs, V, None)
    Cb, Db = (torch.full((M, N + pad), 7.0, device="cuda") for _ in range(2))
    a.eng.spmm_gated_device_rm_bf16(NORM, EPS, N, gin, Cb.data_ptr(), N + pad, Db.data_ptr(), N + pad, None, N, a.stream())
    Gt, work = torch.from_numpy(G).cuda(), torch.zeros((M * N,), device="cuda")
    bufs = {"dxdst": torch.full((M, N + pad), 7.0, device="cuda"), "dxsrc": torch.full((K, N + pad), 7.0, device="cuda"),
            "dv": torch.full((K, N + pad), 7.0, device="cuda")}
    out = sx.api.GatedGrad()
    for k, b in bufs.items():
        setattr(out, "d_" + k, b.data_ptr())
        setattr(out, "ld_" + k, N + pad)
    a.eng.spmm_gated_backward_device_rm_bf16(NORM, EPS, N, gin, Cb.data_ptr(), N + pad, Db.data_ptr(), N + pad, Gt.data_ptr(), N, None, N, out,
                                             work.data_ptr(), a.stream())
    torch.cuda.synchronize()
    for b in [Cb, Db] + list(bufs.values()):
        x = b.cpu().numpy()
        assert np.all(x[:, :N].view(np.uint32) == 0) and np.all(x[:, N:] == 7.0)
    a.eng.close()


# --- determinism -----------------------------------------------------------------------------------------------------------------------------
def test_determinism_streams_and_graph_replay(sx):
    import torch
    N, mode = 24, NORM
    rp, ci, M, K, xd, xs, V, E16, G, Gz16 = case16(N, mode, True)
    a = GatedBf16Abi(sx, rp, ci, M, K)

    def both():
        f = a.fwd16(mode, xd, xs, V, E16)
        g = a.bwd16(mode, xd, xs, V, E16, f, G, Gz16)
        return [f[k] for k in OUT] + [g[k] for k in GRADS]

    def eq(x, y):
        return np.array_equal(x, y) if x.dtype == np.uint16 else same(x, y)

    first, second = both(), both()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = both()
    torch.cuda.current_stream().wait_stream(side)
    for i, (x, y, z) in enumerate(zip(first, second, third)):
        assert eq(x, y) and eq(x, z), i

    # a fresh engine: prepare() alone builds the tables and A^T, then the forward and the backward are captured on a single stream and
    # replayed twice
    b = GatedBf16Abi(sx, rp, ci, M, K)
    b.eng.prepare(N, True, torch.cuda.current_stream().cuda_stream, transposed=True)
    torch.cuda.synchronize()
    gin, keep = b.operands16(xd, xs, V, E16)
    Gt, Gzt = torch.from_numpy(G).cuda(), b.dev16(Gz16, PAD_GZ)
    Ct, Dt, dxd = (torch.zeros((M, N), device="cuda") for _ in range(3))
    dxs, dv = (torch.zeros((K, N), device="cuda") for _ in range(2))
    zt, det = b.out16(b.nnz, N, PAD_Z), b.out16(b.nnz, N, PAD_DE)
    out = sx.api.GatedGrad()
    for k, t, ld in (("dxdst", dxd, N), ("dxsrc", dxs, N), ("dv", dv, N), ("de", det, N + PAD_DE)):
        setattr(out, "d_" + k, t.data_ptr())
        setattr(out, "ld_" + k, ld)
    work = torch.zeros((b.eng.spmm_gated_workspace_floats(mode, N),), device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        s = torch.cuda.current_stream().cuda_stream
        b.eng.spmm_gated_device_rm_bf16(mode, EPS, N, gin, Ct.data_ptr(), N, Dt.data_ptr(), N, zt.data_ptr(), N + PAD_Z, s)
        b.eng.spmm_gated_backward_device_rm_bf16(mode, EPS, N, gin, Ct.data_ptr(), N, Dt.data_ptr(), N, Gt.data_ptr(), N, Gzt.data_ptr(),
                                                 N + PAD_GZ, out, work.data_ptr(), s)
    for _ in range(2):
        for x in (Ct, Dt, dxd, dxs, dv):
            x.zero_()
        zt.fill_(POISON16)
        det.fill_(POISON16)
        g.replay()
        torch.cuda.synchronize()
        zb, deb = b.host16(zt, b.nnz), b.host16(det, b.nnz)
        got = [Ct.cpu().numpy(), Dt.cpu().numpy(), zb[:, :N], dxd.cpu().numpy(), dxs.cpu().numpy(), dv.cpu().numpy(), deb[:, :N]]
        for i, (x, y) in enumerate(zip(got, first)):
            assert eq(x, y), i
        assert untouched(zb, N) and untouched(deb, N)
    a.eng.close()
    b.eng.close()
