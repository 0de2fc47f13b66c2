"""bf16 edge tensors of the two per-channel softmax families on the GPU through the C ABI (sextans_vector_attention_device_rm_bf16 /
_backward_device_rm_bf16, sextans_spmm_edge_softagg_device_rm_bf16 / _backward_device_rm_bf16).  The contract under test: a bf16 value
read is widened exactly, every operation, the online-softmax state and every sum is the fp32 entry point's, in its order; a bf16 value
written is its fp32 result rounded once to nearest even.  So the reference of every comparison is the fp32 entry point ON THE SAME
ENGINE on the widened inputs, and every comparison is on bits:
  fp32 outputs (C, lse, dV, dB, dt)   the twin's bits (same);
  bf16 outputs (dS, dD, dE)           to_bf16(the twin's output) (bf16 NaNs compared as NaNs where special values are planted, same16).
No tolerance anywhere.
  dealing    the 92-row pattern P of test_pattern_dealing_gpu.py and its transpose (long-row kernel, second walk, empty rows) at every
             slot width of the families, N = 8, 16, 32, 64; all modes and ops; the operands of the families' own dealing tests with the
             edge tensors rounded to bf16; and the sharper forward check (S = 0 / t = 0, integer messages, mean_is_exact);
  bits       the 400 x 300 matrix of the reduce tests at N = 8, 24, 72 (one tile; a partial tile; two tiles, the last one partial):
             every gradient alone and all together, a gradient not asked for keeps its sentinel;
  and special values, degenerate matrices and determinism (runs, streams, a graph captured on a fresh prepared engine, replayed twice).
Every bf16 tensor sits in a buffer with a padded leading dimension whose padding holds the pattern 0x5A5A (the scheme of
test_edge_bf16_gpu.py): an input's padding that were read would change a result, an output's padding must come back untouched."""
import numpy as np
import pytest

import test_edge_softagg_dealing_gpu as esd
import test_spmm_edge_softagg_gpu as es
import test_vector_attention_dealing_gpu as vad
import test_vector_attention_gpu as va
from test_bf16_operands_gpu import same16, to_bf16, widen
from test_edge_bf16_gpu import POISON16, Bf16Abi, untouched
from test_fused_attention_gpu import rand, same
from test_pattern_dealing_gpu import int_values, mean_is_exact, pat, rng
from test_spmm_edge_softagg_gpu import OPS
from test_spmm_softagg_gpu import cut_rows
from test_vector_attention_gpu import MODES, VattAbi, grads_of, scores

pytestmark = pytest.mark.gpu

WIDTHS = [8, 16, 32, 64]
SIZES = [8, 24, 72]
PAD_S, PAD_D, PAD_DS, PAD_DD, PAD_E, PAD_DE = 4, 8, 12, 4, 4, 8   # extra columns of the bf16 buffers (leading dimensions: multiples of 4)
EGRADS = es.GRADS                                                 # dB dE dt
NAN16, INF16, NINF16, NZERO16 = 0x7FC0, 0x7F80, 0xFF80, 0x8000


class SoftBf16Abi(VattAbi):
    """one engine on a pattern: the four bf16 entry points, and their fp32 twins (VattAbi.fwd / .bwd, es.EdgeSoftAbi.fwd / .bwd) on the
    same engine"""
    dev16, out16, host16 = Bf16Abi.dev16, Bf16Abi.out16, staticmethod(Bf16Abi.host16)

    def __init__(self, sx, rp, ci, M, K):
        super().__init__(sx, rp, ci, np.ones(len(ci), np.float32), M, K)

    def stream(self):
        return self.t.cuda.current_stream().cuda_stream

    # --- vector attention ---
    def vfwd16(self, mode, S16, V, D16, want_lse=True):
        """-> (C, lse) fp32; C and lse start as 7.0 (lse keeps it when it is not asked for)"""
        tc = self.t
        N = S16.shape[1]
        Sb, Vb, Db = self.dev16(S16, PAD_S), self.dev(V), self.dev16(D16, PAD_D)
        Cb, Lb = (tc.full((max(self.M, 1), N), 7.0, device="cuda") for _ in range(2))
        ptr = lambda x: x.data_ptr() if x is not None else None   # noqa: E731
        self.eng.vector_attention_device_rm_bf16(MODES[mode], N, ptr(Sb), N + PAD_S, ptr(Vb), N, ptr(Db), N + PAD_D, Cb.data_ptr(), N,
                                                 Lb.data_ptr() if want_lse else None, N, self.stream())
        tc.cuda.synchronize()
        return Cb.cpu().numpy()[:self.M], Lb.cpu().numpy()[:self.M]

    def vbwd16(self, mode, S16, V, D16, C, lse, G, want=va.GRADS):
        """-> {dS, dD: uint16 (nnz, N); dV: fp32; dSb, dDb: the whole padded buffers}; a gradient not in `want` gets no pointer and keeps
        its sentinel (POISON16 / 7.0)"""
        tc = self.t
        N = G.shape[1]
        Sb, Vb, Db = self.dev16(S16, PAD_S), self.dev(V), self.dev16(D16, PAD_D)
        Cb, Lb, Gb = (self.dev(x) for x in (C, lse, G))
        dS, dD = self.out16(self.nnz, N, PAD_DS), self.out16(self.nnz, N, PAD_DD)
        dV = tc.full((self.K, N), 7.0, device="cuda")
        p = {k: (x.data_ptr() if k in want else None) for k, x in (("dS", dS), ("dV", dV), ("dD", dD))}
        ptr = lambda x: x.data_ptr() if x is not None else None   # noqa: E731
        self.eng.vector_attention_backward_device_rm_bf16(MODES[mode], N, ptr(Sb), N + PAD_S, ptr(Vb), N, ptr(Db), N + PAD_D, ptr(Cb), N,
                                                          ptr(Lb), N, ptr(Gb), N, p["dS"], N + PAD_DS, p["dV"], N, p["dD"], N + PAD_DD,
                                                          self.stream())
        tc.cuda.synchronize()
        dSb, dDb = self.host16(dS, self.nnz), self.host16(dD, self.nnz)
        return {"dS": dSb[:, :N], "dD": dDb[:, :N], "dV": dV.cpu().numpy(), "dSb": dSb, "dDb": dDb}

    def vfwd32(self, mode, S16, V, D16):
        return VattAbi.fwd(self, mode, widen(S16), V, widen(D16) if D16 is not None else None)[:2]

    def vbwd32(self, mode, S16, V, D16, C, lse, G, want=va.GRADS):
        return VattAbi.bwd(self, mode, widen(S16), V, widen(D16) if D16 is not None else None, C, lse, G, want=want)

    # --- edge softagg ---
    def sfwd16(self, op, B, E16, t, want_lse=True):
        tc = self.t
        N = E16.shape[1]
        Bb = self.dev(B) if op != "copy" else None
        Eb = self.dev16(E16, PAD_E)
        tt = tc.from_numpy(t).cuda() if t is not None else None
        Cb, Lb = (tc.full((max(self.M, 1), N), 7.0, device="cuda") for _ in range(2))
        ptr = lambda x: x.data_ptr() if x is not None else None   # noqa: E731
        self.eng.spmm_edge_softagg_device_rm_bf16(OPS[op], N, ptr(Bb), N, Eb.data_ptr(), N + PAD_E, ptr(tt), Cb.data_ptr(), N,
                                                  Lb.data_ptr() if want_lse else None, N, self.stream())
        tc.cuda.synchronize()
        return Cb.cpu().numpy()[:self.M], Lb.cpu().numpy()[:self.M]

    def sbwd16(self, op, B, E16, t, C, lse, G, want=EGRADS):
        """-> {dB, dt: fp32; dE: uint16 (nnz, N); dEb: its whole padded buffer}; a gradient not in `want` gets no pointer and keeps its
        sentinel; the workspace is the twin's"""
        tc = self.t
        N = G.shape[1]
        Bb = self.dev(B) if op != "copy" else None
        Eb = self.dev16(E16, PAD_E)
        tt = tc.from_numpy(t).cuda() if t is not None else None
        Cb, Lb, Gb = (self.dev(x) for x in (C, lse, G))
        nwork = self.eng.spmm_edge_softagg_workspace_floats(N)
        dB, dt, work = tc.full((self.K, N), 7.0, device="cuda"), tc.full((N,), 7.0, device="cuda"), tc.full((max(nwork, 1),), 7.0, device="cuda")
        dE = self.out16(self.nnz, N, PAD_DE)
        p = {k: (x.data_ptr() if k in want else None) for k, x in (("dB", dB), ("dE", dE), ("dt", dt))}
        ptr = lambda x: x.data_ptr() if x is not None else None   # noqa: E731
        self.eng.spmm_edge_softagg_backward_device_rm_bf16(OPS[op], N, ptr(Bb), N, Eb.data_ptr(), N + PAD_E, ptr(tt), ptr(Cb), N, ptr(Lb), N,
                                                           ptr(Gb), N, p["dB"], N, p["dE"], N + PAD_DE, p["dt"], work.data_ptr(), self.stream())
        tc.cuda.synchronize()
        dEb = self.host16(dE, self.nnz)
        return {"dB": dB.cpu().numpy(), "dE": dEb[:, :N], "dt": dt.cpu().numpy(), "dEb": dEb}

    def sfwd32(self, op, B, E16, t):
        return es.EdgeSoftAbi.fwd(self, op, B, widen(E16), t)[:2]

    def sbwd32(self, op, B, E16, t, C, lse, G, want=EGRADS):
        return es.EdgeSoftAbi.bwd(self, op, B, widen(E16), t, C, lse, G, want=want)


def egrads_of(op):
    return [g for g in EGRADS if not (op == "copy" and g == "dB")]


def vatt_matches(a, mode, S16, V, D16, G, names=None, nan=False):
    """forward and backward of one mode on both entry points: fp32 outputs the twin's bits, bf16 outputs its outputs rounded; the
    gradients not in `names` keep their sentinels.  -> (C, lse, the bf16 run's gradients, the twin's, the two last_kernels of the bf16 run)"""
    names = grads_of(mode) if names is None else names
    eq16 = same16 if nan else np.array_equal
    C, lse = a.vfwd16(mode, S16, V, D16)
    fwd = a.eng.last_kernel()
    rC, rL = a.vfwd32(mode, S16, V, D16)
    assert a.eng.last_kernel() == fwd.replace("_bf16", "")
    assert same(C, rC) and same(lse, rL), mode
    got = a.vbwd16(mode, S16, V, D16, C, lse, G, want=names)
    bwd = a.eng.last_kernel()
    ref = a.vbwd32(mode, S16, V, D16, C, lse, G, want=names)
    assert a.eng.last_kernel() == bwd.replace("_bf16", "")
    for g, buf in (("dS", "dSb"), ("dD", "dDb")):
        if g in names:
            assert eq16(got[g], to_bf16(ref[g])) and untouched(got[buf], G.shape[1]), (mode, g)
        else:
            assert np.all(got[buf] == POISON16) and np.all(ref[g] == 7.0), (mode, g)
    assert same(got["dV"], ref["dV"]), mode          # (not asked for: 7.0 in both)
    return C, lse, got, ref, (fwd, bwd)


def soft_matches(a, op, B, E16, t, G, names=None, nan=False):
    """the same for one op of the edge softagg; dt is bit-equal to the twin's"""
    names = egrads_of(op) if names is None else names
    eq16 = same16 if nan else np.array_equal
    C, lse = a.sfwd16(op, B, E16, t)
    fwd = a.eng.last_kernel()
    rC, rL = a.sfwd32(op, B, E16, t)
    assert a.eng.last_kernel() == fwd.replace("_bf16", "")
    assert same(C, rC) and same(lse, rL), op
    got = a.sbwd16(op, B, E16, t, C, lse, G, want=names)
    bwd = a.eng.last_kernel()
    ref = a.sbwd32(op, B, E16, t, C, lse, G, want=names)
    assert a.eng.last_kernel() == bwd.replace("_bf16", "")
    if "dE" in names:
        assert eq16(got["dE"], to_bf16(ref["dE"])) and untouched(got["dEb"], G.shape[1]), op
    else:
        assert np.all(got["dEb"] == POISON16) and np.all(ref["dE"] == 7.0), op
    assert same(got["dB"], ref["dB"]) and same(got["dt"], ref["dt"]), op
    return C, lse, got, ref, (fwd, bwd)


def bf16_names(names):
    """the twins' names_ok on the bf16 names with the suffix taken out: _bf16 sits between the family's name and +long_rows"""
    for n in names:
        assert "_bf16" in n and (n.endswith("_bf16") or n.endswith("_bf16+long_rows")), n
    return [n.replace("_bf16", "") for n in names]


# --- dealing: every path, every width -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["P", "PT"])
@pytest.mark.parametrize("N", WIDTHS)
def test_vector_attention_on_every_dealing_path(sx, N, name):
    p = pat(name)
    a = SoftBf16Abi(sx, p.rp, p.ci, p.M, p.K)
    for mode in MODES:
        S, V, D, G = vad.operands(rng("vector_attention", mode, N, name), p, N)
        S16, D16 = to_bf16(S), to_bf16(D)
        _, _, got, ref, kernels = vatt_matches(a, mode, S16, V, D16, G)
        vad.names_ok(p, mode, *bf16_names(kernels))
        assert np.any(widen(got["dS"]) != ref["dS"])          # (the rounding is not vacuous)
    # the sharper forward check: S = 0 and integer messages exact in bf16, every weight 1 / n
    rs = rng("u-vector_attention-bf16", N, name)
    sign = lambda *shape: rs.choice([-1, 1], shape).astype(np.float32)   # noqa: E731
    cases = {"node": (int_values(rs, p.K, N), None),
             "add": ((rs.randint(3, 5, (p.K, N)) * sign(p.K, N)).astype(np.float32), sign(p.nnz, N)),
             "edge": (None, int_values(rs, p.nnz, N))}
    S16 = np.zeros((p.nnz, N), np.uint16)
    for mode, (V, D) in cases.items():
        D16 = to_bf16(D) if D is not None else None
        assert D is None or np.array_equal(widen(D16), D)
        C, lse = a.vfwd16(mode, S16, V, D16)
        assert a.eng.last_kernel() == "vector_attention_bf16" + ("+long_rows" if p.long_rows else "")
        m = va.messages32(mode, V, D, p.ci)
        assert np.abs(m).max() <= 5
        mean_is_exact(p, C, lse, m)
    a.eng.close()


@pytest.mark.parametrize("name", ["P", "PT"])
@pytest.mark.parametrize("N", WIDTHS)
def test_edge_softagg_on_every_dealing_path(sx, N, name):
    p = pat(name)
    a = SoftBf16Abi(sx, p.rp, p.ci, p.M, p.K)
    for op in OPS:
        B, E, G, t = esd.operands(rng("edge_softagg", op, N, name), p, N)
        E16 = to_bf16(E)
        _, _, got, ref, kernels = soft_matches(a, op, B, E16, t, G)
        esd.names_ok(p, op, *bf16_names(kernels))
        assert np.any(widen(got["dE"]) != ref["dE"])
    rs = rng("u-edge_softagg-bf16", N, name)
    sign = lambda *shape: rs.choice([-1, 1], shape).astype(np.float32)   # noqa: E731
    cases = {"mul": (int_values(rs, p.K, N), sign(p.nnz, N)),
             "add": ((rs.randint(3, 5, (p.K, N)) * sign(p.K, N)).astype(np.float32), sign(p.nnz, N)),
             "copy": (None, int_values(rs, p.nnz, N))}
    for op, (B, E) in cases.items():
        E16 = to_bf16(E)
        assert np.array_equal(widen(E16), E)
        C, lse = a.sfwd16(op, B, E16, np.zeros(N, np.float32))
        assert a.eng.last_kernel() == "spmm_edge_softagg_bf16" + ("+long_rows" if p.long_rows else "")
        m = es.messages32(op, B, E, p.ci)
        assert np.abs(m).max() <= 5
        mean_is_exact(p, C, lse, m)
    a.eng.close()


# --- bits on the 400 x 300 matrix ---------------------------------------------------------------------------------------------------------
_cases = {}


def base_case(N):
    """the 400 x 300 matrix of the reduce tests (empty rows, one row of 300): the operands of the families' own tests, the edge tensors
    rounded to bf16; once per N, never changed"""
    if N not in _cases:
        rp, ci, _, M, K, S, V, D, G = va.inputs(N)
        E = es.inputs(N)[6]
        _cases[N] = (rp, ci, M, K, to_bf16(S), V, to_bf16(D), G, to_bf16(E), es.temps(N))
    return _cases[N]


@pytest.mark.parametrize("N", SIZES)
def test_vector_attention_has_the_bits_of_the_fp32_entry_on_the_widened_inputs(sx, N):
    rp, ci, M, K, S16, V, D16, G, _, _ = base_case(N)
    a = SoftBf16Abi(sx, rp, ci, M, K)
    for mode in MODES:
        names = grads_of(mode)
        C, lse, got, ref, kernels = vatt_matches(a, mode, S16, V, D16, G)
        assert kernels == ("vector_attention_bf16", "vector_attention_backward_bf16")
        assert np.any(widen(got["dS"]) != ref["dS"])
        for g in names:                      # each gradient alone: the same bits, the others' buffers untouched
            _, _, alone, _, _ = vatt_matches(a, mode, S16, V, D16, G, names=(g,))
            assert np.array_equal(alone[g], got[g]) if g != "dV" else same(alone[g], got[g]), (mode, g)
        C2, lse2 = a.vfwd16(mode, S16, V, D16, want_lse=False)   # inference: no lse, the same C
        assert same(C2, C) and np.all(lse2 == 7.0)
    a.eng.close()


@pytest.mark.parametrize("N", SIZES)
def test_edge_softagg_has_the_bits_of_the_fp32_entry_on_the_widened_inputs(sx, N):
    rp, ci, M, K, _, B, _, G, E16, t = base_case(N)
    a = SoftBf16Abi(sx, rp, ci, M, K)
    for op in OPS:
        for tt in (t, None):                 # the temperatures, and the kernels' t == NULL path
            C, lse, got, ref, kernels = soft_matches(a, op, B, E16, tt, G)
            assert kernels == ("spmm_edge_softagg_bf16", "spmm_edge_softagg_backward_bf16")
            assert np.any(widen(got["dE"]) != ref["dE"])
        for g in egrads_of(op):
            _, _, alone, _, _ = soft_matches(a, op, B, E16, t, G, names=(g,))
        C2, lse2 = a.sfwd16(op, B, E16, None, want_lse=False)
        assert same(C2, C) and np.all(lse2 == 7.0)
    a.eng.close()


# --- special values ---------------------------------------------------------------------------------------------------------------------------
BIG_G = np.array([0x7F7FC000], np.uint32).view(np.float32)[0]   # finite in fp32, above bf16's rounding boundary 0x7F7F8000


def quiet(b16):
    """every NaN among these bf16 patterns is a quiet one"""
    nan = np.isnan(widen(b16))
    return bool(np.all(b16[nan] & 0x40))


def test_masks_in_bf16_scores(sx):
    """a bf16 -inf score is still a mask: weight +0 and dS exactly +0 (the bits).  All scores of one (row, column) -inf: NaN in C there
    and nowhere else, lse = -inf; the mask rule gives dS = +0 there too, and the NaN weight shows in dD = G w, as a quiet NaN in bf16"""
    N, mode = 24, "add"
    rp, ci, M, K, S16, V, D16, G, _, _ = base_case(N)
    rows = es.rows_of(rp)
    rs = np.random.RandomState(31)
    mask = rs.rand(*S16.shape) < 1.0 / 3
    mask[rp[:-1][np.diff(rp) > 0]] = False           # no (row, column) fully masked here: the first entry of every row stays
    S2 = S16.copy()
    S2[mask] = NINF16
    a = SoftBf16Abi(sx, rp, ci, M, K)
    C, lse, got, ref, _ = vatt_matches(a, mode, S2, V, D16, G)
    assert np.all(np.isfinite(C)) and mask.sum() > 1000
    assert np.all(got["dS"][mask] == 0)                                            # +0, not G's sign
    assert np.all(got["dD"][mask] & 0x7FFF == 0)                                   # G w with a weight of exactly +0 ...
    assert np.all(got["dD"][mask & (G[rows] > 0)] == 0)                            # ... +0 where G is positive
    # one (row, column) fully masked
    r0, n0 = int(np.flatnonzero(np.diff(rp) == 300)[0]), 19
    S3 = S16.copy()
    S3[rp[r0]:rp[r0 + 1], n0] = NINF16
    C3, lse3, got3, ref3, _ = vatt_matches(a, mode, S3, V, D16, G, nan=True)
    hit = np.zeros((M, N), bool)
    hit[r0, n0] = True
    assert np.array_equal(np.isnan(C3), hit) and lse3[r0, n0] == -np.inf
    ehit = np.zeros(S16.shape, bool)
    ehit[rp[r0]:rp[r0 + 1], n0] = True
    assert np.all(got3["dS"][ehit] == 0)
    assert np.array_equal(np.isnan(widen(got3["dD"])), ehit) and np.array_equal(np.isnan(ref3["dD"]), ehit) and quiet(got3["dD"])
    a.eng.close()


def test_special_values_stay_in_their_entry_row_and_column(sx):
    """NaN, +-inf and -0 in D / E: each shows in its own (entry, column), in the row (C, lse) and the column (dV, dB) that hold it, and
    nowhere else -- the twin's pattern, and the twin's bits wherever the value is not a NaN; a bf16 NaN is a quiet one"""
    N = 24
    rp, ci, M, K, S16, V, D16, G, E16, t = base_case(N)
    rows = es.rows_of(rp)
    e1 = len(ci) // 3
    cols = [3, 17, 20, 6]
    D2, E2 = D16.copy(), E16.copy()
    D2[e1, cols] = NAN16, INF16, NINF16, NZERO16
    E2[e1, cols] = NAN16, INF16, NINF16, NZERO16
    a = SoftBf16Abi(sx, rp, ci, M, K)
    for mode in ("add", "edge"):
        C, lse, got, ref, _ = vatt_matches(a, mode, S16, V, D2, G, nan=True)
        bad = ~np.isfinite(C)
        assert bad[rows[e1], cols[:3]].all() and not np.delete(bad, rows[e1], axis=0).any(), mode   # the row of the entry, nowhere else
        assert np.all(np.isfinite(lse[np.diff(rp) > 0]))                                            # (the scores are finite)
        assert np.isnan(widen(got["dS"][e1, cols[:1]]))[0] and quiet(got["dS"]) and quiet(got["dD"])
        assert not np.delete(~np.isfinite(widen(got["dS"])), np.arange(rp[rows[e1]], rp[rows[e1] + 1]), axis=0).any(), mode
        if mode == "add":
            assert np.all(np.isfinite(got["dV"]))                                                   # dV = sum G w: no message in it
    for op in OPS:
        C, lse, got, ref, _ = soft_matches(a, op, B=V, E16=E2, t=t, G=G, nan=True)
        bad = ~np.isfinite(C)
        assert bad[rows[e1], cols[0]] and not np.delete(bad, rows[e1], axis=0).any(), op
        assert quiet(got["dE"])
        assert not np.delete(~np.isfinite(widen(got["dE"])), np.arange(rp[rows[e1]], rp[rows[e1] + 1]), axis=0).any(), op
        if op != "copy":
            badB = np.flatnonzero(~np.isfinite(got["dB"]).all(axis=1))
            assert set(badB) <= set(ci[rp[rows[e1]]:rp[rows[e1] + 1]].tolist()), op                 # only columns of that row's entries
    # -0 stays -0 through a write: dD = G w with G = -0 on a row
    G2 = G.copy()
    G2[rows[e1]] = -0.0
    _, _, got, _, _ = vatt_matches(a, "edge", S16, None, D16, G2)
    assert np.all(got["dD"][rp[rows[e1]]:rp[rows[e1] + 1]] == NZERO16)
    a.eng.close()


def test_a_gradient_above_bf16_range_becomes_inf(sx):
    """rows of one entry: the weight is exactly 1, so dD = G and dE = q = G (m - C = 0).  G = 0x7F7FC000 is finite in fp32 and at or above
    bf16's rounding boundary: inf in bf16, only there"""
    N = 24
    rp, ci, M, K, S16, V, D16, G, E16, _ = base_case(N)
    kept = np.arange(len(ci))
    rp1, ci1, kept = cut_rows(rp, ci, kept)
    single = np.flatnonzero(np.diff(rp1) == 1)
    assert len(single) >= 40
    r0, n0 = int(single[5]), 9
    e0 = int(rp1[r0])
    G2 = G.copy()
    G2[r0, n0] = BIG_G
    a = SoftBf16Abi(sx, rp1, ci1, M, K)
    hit = np.zeros((len(ci1), N), bool)
    hit[e0, n0] = True
    for mode in ("add", "edge"):
        _, _, got, ref, _ = vatt_matches(a, mode, S16[kept], V, D16[kept], G2)
        assert np.isfinite(ref["dD"][e0, n0]) and ref["dD"][e0, n0] == BIG_G and got["dD"][e0, n0] == INF16, mode
        assert np.array_equal(~np.isfinite(widen(got["dD"])), hit), mode
    for op in ("add", "copy"):
        _, _, got, ref, _ = soft_matches(a, op, V, E16[kept], None, G2)
        assert np.isfinite(ref["dE"][e0, n0]) and ref["dE"][e0, n0] == BIG_G and got["dE"][e0, n0] == INF16, op
        assert np.array_equal(~np.isfinite(widen(got["dE"])), hit), op
    a.eng.close()


# --- degenerate matrices -------------------------------------------------------------------------------------------------------------------
def test_degenerate_matrices(sx):
    """no rows, and no entries: OK, dS, dD and dE have no element, C, dV, dB and dt are zeroed, lse = -inf, last_kernel stays what it was"""
    N = 16
    rs = np.random.RandomState(4)
    for M, K in ((0, 7), (9, 7)):
        rp, ci = np.zeros(M + 1, np.int32), np.zeros(0, np.int32)
        V, G, none16 = rand(rs, K, N), rand(rs, M, N), np.zeros((0, N), np.uint16)
        a = SoftBf16Abi(sx, rp, ci, M, K)
        before = a.eng.last_kernel()
        zeros = lambda x, shape: x.shape == shape and np.all(np.ascontiguousarray(x).view(np.uint32) == 0)   # noqa: E731
        for mode in MODES:
            C, lse = a.vfwd16(mode, none16, V, none16)
            assert zeros(C, (M, N)) and lse.shape == (M, N) and np.all(lse == -np.inf), mode
            got = a.vbwd16(mode, none16, V, none16, C, lse, G, want=grads_of(mode))
            assert got["dS"].shape == (0, N) and got["dD"].shape == (0, N)
            if mode != "edge":
                assert zeros(got["dV"], (K, N)), mode
        for op in OPS:
            C, lse = a.sfwd16(op, V, none16, None)
            assert zeros(C, (M, N)) and np.all(lse == -np.inf), op
            got = a.sbwd16(op, V, none16, None, C, lse, G, want=egrads_of(op))
            assert got["dE"].shape == (0, N) and zeros(got["dt"], (N,)), op
            if op != "copy":
                assert zeros(got["dB"], (K, N)), op
        assert a.eng.last_kernel() == before
        a.eng.close()


# --- determinism -----------------------------------------------------------------------------------------------------------------------------
def test_determinism_streams_and_graph_replay(sx):
    import torch
    N, mode, op = 24, "add", "add_relu"
    rp, ci, M, K, S16, V, D16, G, E16, t = base_case(N)
    a = SoftBf16Abi(sx, rp, ci, M, K)

    def all_four():
        C, lse = a.vfwd16(mode, S16, V, D16)
        g = a.vbwd16(mode, S16, V, D16, C, lse, G)
        C2, lse2 = a.sfwd16(op, V, E16, t)
        h = a.sbwd16(op, V, E16, t, C2, lse2, G)
        return [C, lse, g["dS"], g["dV"], g["dD"], C2, lse2, h["dB"], h["dE"], h["dt"]]

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
    b = SoftBf16Abi(sx, rp, ci, M, K)
    b.eng.prepare(N, True, torch.cuda.current_stream().cuda_stream, transposed=True)
    torch.cuda.synchronize()
    Vt, Gt, tt = b.dev(V), b.dev(G), torch.from_numpy(t).cuda()
    St, Dt, Et = b.dev16(S16, PAD_S), b.dev16(D16, PAD_D), b.dev16(E16, PAD_E)
    dSt, dDt, dEt = b.out16(b.nnz, N, PAD_DS), b.out16(b.nnz, N, PAD_DD), b.out16(b.nnz, N, PAD_DE)
    Ct, Lt, C2t, L2t = (torch.zeros((M, N), device="cuda") for _ in range(4))
    dVt, dBt = (torch.zeros((K, N), device="cuda") for _ in range(2))
    dtt, work = torch.zeros((N,), device="cuda"), torch.zeros((b.eng.spmm_edge_softagg_workspace_floats(N),), device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        s = torch.cuda.current_stream().cuda_stream
        b.eng.vector_attention_device_rm_bf16(MODES[mode], N, St.data_ptr(), N + PAD_S, Vt.data_ptr(), N, Dt.data_ptr(), N + PAD_D,
                                              Ct.data_ptr(), N, Lt.data_ptr(), N, s)
        b.eng.vector_attention_backward_device_rm_bf16(MODES[mode], N, St.data_ptr(), N + PAD_S, Vt.data_ptr(), N, Dt.data_ptr(), N + PAD_D,
                                                       Ct.data_ptr(), N, Lt.data_ptr(), N, Gt.data_ptr(), N, dSt.data_ptr(), N + PAD_DS,
                                                       dVt.data_ptr(), N, dDt.data_ptr(), N + PAD_DD, s)
        b.eng.spmm_edge_softagg_device_rm_bf16(OPS[op], N, Vt.data_ptr(), N, Et.data_ptr(), N + PAD_E, tt.data_ptr(), C2t.data_ptr(), N,
                                               L2t.data_ptr(), N, s)
        b.eng.spmm_edge_softagg_backward_device_rm_bf16(OPS[op], N, Vt.data_ptr(), N, Et.data_ptr(), N + PAD_E, tt.data_ptr(), C2t.data_ptr(),
                                                        N, L2t.data_ptr(), N, Gt.data_ptr(), N, dBt.data_ptr(), N, dEt.data_ptr(), N + PAD_DE,
                                                        dtt.data_ptr(), work.data_ptr(), s)
    for _ in range(2):
        for x in (Ct, Lt, dSt, dVt, dDt, C2t, L2t, dBt, dEt, dtt):
            x.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = [Ct.cpu().numpy(), Lt.cpu().numpy(), b.host16(dSt, b.nnz)[:, :N], dVt.cpu().numpy(), b.host16(dDt, b.nnz)[:, :N],
               C2t.cpu().numpy(), L2t.cpu().numpy(), dBt.cpu().numpy(), b.host16(dEt, b.nnz)[:, :N], dtt.cpu().numpy()]
        for i, (x, y) in enumerate(zip(got, first)):
            assert eq(x, y), i
    a.eng.close()
    b.eng.close()
