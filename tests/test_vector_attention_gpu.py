"""Channel-wise attention from per-channel scores on the GPU through the C ABI (sextans_vector_attention_device_rm / _backward_device_rm):
C, lse, dS, dV and dD against a float64 numpy reference built row by row from the fp32-rounded messages; every subset of the gradients;
exact bits where the arithmetic fixes them (empty rows, rows of one entry, S = t m against spmm_edge_softagg and spmm_softagg); -inf
scores as masks; padded leading dimensions; determinism across runs, streams and a graph replay; degenerate matrices.

Tolerance: test_torch_autograd_gpu._close (rtol 2e-4), the project's tolerance for fp32 sums.  Operands: the 400 x 300 matrix of
test_spmm_edge_softagg_gpu.inputs with V and D uniform in +-1 and the scores S uniform in +-4 (scores()).  emulate() below restates the
kernels' fp32 arithmetic on the CPU (one entry after the other) and tests/test_vector_attention_tolerance.py (no GPU) holds it against
the reference on these inputs at N = 16.  Largest error / limit per mode:
    node 0.045 (dS)    add 0.045 (dS)    edge 0.074 (dS)        (C <= 0.020, lse <= 0.004, dV <= 0.043, dD <= 0.004 everywhere)
-- all below 0.5, so no mode's inputs are shrunk."""
import numpy as np
import pytest

import test_spmm_edge_softagg_gpu as es
from test_fused_attention_gpu import rand, same
from test_pattern_dealing_gpu import pat
from test_spmm_edge_softagg_gpu import limit_ratio, rows_of
from test_spmm_reduce_gpu import POISON, Abi, bits_equal
from test_spmm_softagg_gpu import SoftAbi, cut_rows, lse_close, temps
from test_torch_autograd_gpu import _close

pytestmark = pytest.mark.gpu

MODES = {"node": 1, "add": 2, "edge": 3}   # SEXTANS_VATT_*
GRADS = ("dS", "dV", "dD")
SIZES = [8, 16, 24, 72]                    # one tile; a partial tile (24); two tiles, the last one partial (72)


def grads_of(mode):
    return [g for g in GRADS if not (mode == "edge" and g == "dV") and not (mode == "node" and g == "dD")]


def messages32(mode, V, D, ci):
    """(nnz, N) float32: the kernels' messages, at most one rounded operation each"""
    m = V[ci] if mode == "node" else D if mode == "edge" else V[ci] + D
    assert m.dtype == np.float32
    return m


def scores(seed, nnz, N, scale=4.0):
    """the (nnz, N) scores: uniform in +-scale"""
    return rand(np.random.RandomState(seed), nnz, N) * np.float32(scale)


def reference(mode, rp, ci, S, V, D, G=None, K=None):
    """float64, row by row, from the fp32-rounded messages: (C, lse) or, with G, (C, lse, dS, dV, dD); dV None for edge, dD None for
    node.  A score of -inf has weight 0; a (row, column) of only -inf is NaN in C."""
    M, N = len(rp) - 1, S.shape[1]
    m = messages32(mode, V, D, ci).astype(np.float64)
    s = S.astype(np.float64)
    C, lse = np.zeros((M, N)), np.full((M, N), -np.inf)
    gw, dS = np.zeros_like(m), np.zeros_like(m)
    with np.errstate(invalid="ignore", divide="ignore"):
        for r in range(M):
            b, e = rp[r], rp[r + 1]
            if e == b:
                continue
            mx = s[b:e].max(0)
            w = np.exp(s[b:e] - mx)
            z = w.sum(0)
            w /= z
            C[r] = (w * m[b:e]).sum(0)
            lse[r] = np.where(mx == -np.inf, -np.inf, mx + np.log(z))
            if G is not None:
                gw[b:e] = G[r].astype(np.float64) * w
                dS[b:e] = np.where(s[b:e] == -np.inf, 0.0, gw[b:e] * (m[b:e] - C[r]))
    if G is None:
        return C, lse
    dV = None
    if mode != "edge":
        dV = np.zeros((K, N))
        np.add.at(dV, ci, gw)
    return C, lse, dS, dV, (gw if mode != "node" else None)


def emulate(mode, rp, ci, S, V, D, G, K, slots=1):
    """The kernels' arithmetic in float32 on the CPU: (C, lse, dS, dV, dD).  One entry order: a row's entries one after the other
    (slots = 1) or, for a row of at least 2 * slots entries, dealt to `slots` partial states (entry k to state k % slots, as
    pattern_pass.h deals a row to its slots), which a pairwise tree then merges with the kernels' combine.  dV adds a column's entries one
    after the other.  fma is one rounding of the float64 expression; exp and log are numpy's float32 ones."""
    f32, f64 = np.float32, np.float64
    M, N = len(rp) - 1, S.shape[1]
    fma = lambda x, y, z: (x.astype(f64) * y.astype(f64) + np.asarray(z, f64)).astype(f32)   # noqa: E731
    m, s = messages32(mode, V, D, ci), S.astype(f32)
    C, lse = np.zeros((M, N), f32), np.full((M, N), -np.inf, f32)
    with np.errstate(all="ignore"):
        for r in range(M):
            b, e = rp[r], rp[r + 1]
            if e == b:
                continue
            n = slots if e - b >= 2 * slots else 1
            steps = -(-(e - b) // n)
            pos = b + np.arange(steps * n).reshape(steps, n)
            ok, pos = pos < e, np.minimum(pos, e - 1)
            mx, z, acc = np.full((n, N), -np.inf, f32), np.zeros((n, N), f32), np.zeros((n, N), f32)
            for k in range(steps):
                sk, mk = np.where(ok[k][:, None], s[pos[k]], f32(-np.inf)), m[pos[k]]
                mn = np.maximum(mx, sk)
                ref = np.where(mn == -np.inf, f32(0), mn)
                al, w = np.exp(mx - ref), np.exp(sk - ref)
                z, acc, mx = z * al + w, fma(w, mk, acc * al), mn
            while n > 1:   # the tree: state j with state j + n / 2
                n //= 2
                mn = np.maximum(mx[:n], mx[n:])
                ref = np.where(mn == -np.inf, f32(0), mn)
                ca, cb = np.exp(mx[:n] - ref), np.exp(mx[n:] - ref)
                z, acc, mx = z[:n] * ca + z[n:] * cb, acc[:n] * ca + acc[n:] * cb, mn
            C[r], lse[r] = acc[0] / z[0], mx[0] + np.log(z[0])
        rows = rows_of(rp)
        gw = G[rows] * np.exp(s - lse[rows])
        dS = np.where(s == -np.inf, f32(0), gw * (m - C[rows]))
        assert gw.dtype == f32 and dS.dtype == f32
        dV = None
        if mode != "edge":
            dV = np.zeros((K, N), f32)
            np.add.at(dV, ci, gw)          # (float32 adds, in entry order)
    return C, lse, dS, dV, (gw if mode != "node" else None)


class VattAbi(Abi):
    """test_spmm_reduce_gpu.Abi's engine on a matrix, the vector attention's entry points called through api.Engine"""

    def dev(self, x, pad=0, rows=None):
        """a numpy (rows, N) operand in a device buffer `pad` columns wider, or None"""
        if x is None:
            return None
        tc = self.t
        buf = tc.zeros((max(x.shape[0] if rows is None else rows, 1), x.shape[1] + pad), device="cuda")
        buf[:x.shape[0], :x.shape[1]] = tc.from_numpy(np.ascontiguousarray(x))
        return buf

    def fwd(self, mode, S, V, D, want_lse=True, pad=(0, 0, 0, 0, 0)):
        """-> (C, lse) as numpy and the whole padded buffers as int32; pad: extra columns of the S / V / D / C / lse buffers.  The operand
        the mode does not read may be None."""
        tc = self.t
        N = S.shape[1]
        Sb, Vb, Db = self.dev(S, pad[0]), self.dev(V, pad[1]), self.dev(D, pad[2])
        Cb = tc.full((max(self.M, 1), N + pad[3]), POISON, dtype=tc.int32, device="cuda")
        Lb = tc.full((max(self.M, 1), N + pad[4]), POISON, dtype=tc.int32, device="cuda")
        ptr = lambda x: x.data_ptr() if x is not None else None   # noqa: E731
        self.eng.vector_attention_device_rm(MODES[mode], N, ptr(Sb), N + pad[0], ptr(Vb), N + pad[1], ptr(Db), N + pad[2], Cb.data_ptr(),
                                            N + pad[3], Lb.data_ptr() if want_lse else None, N + pad[4], tc.cuda.current_stream().cuda_stream)
        tc.cuda.synchronize()
        Cn, Ln = Cb.cpu().numpy()[:self.M], Lb.cpu().numpy()[:self.M]
        return Cn[:, :N].view(np.float32), Ln[:, :N].view(np.float32), Cn, Ln

    def bwd(self, mode, S, V, D, C, lse, G, want=GRADS, pad=0):
        """-> {name: numpy} of the three gradients, each in a buffer `pad` columns wider that held 7.0: the ones not in `want` get no
        pointer and must keep their 7.0"""
        tc = self.t
        N = G.shape[1]
        Sb, Vb, Db, Cb, Lb, Gb = (self.dev(x) for x in (S, V, D, C, lse, G))
        buf = {"dS": tc.full((max(self.nnz, 1), N + pad), 7.0, device="cuda"), "dV": tc.full((self.K, N + pad), 7.0, device="cuda"),
               "dD": tc.full((max(self.nnz, 1), N + pad), 7.0, device="cuda")}
        p = {k: (x.data_ptr() if k in want else None) for k, x in buf.items()}
        ptr = lambda x: x.data_ptr() if x is not None else None   # noqa: E731
        self.eng.vector_attention_backward_device_rm(MODES[mode], N, ptr(Sb), N, ptr(Vb), N, ptr(Db), N, ptr(Cb), N, ptr(Lb), N, ptr(Gb), N,
                                                     p["dS"], N + pad, p["dV"], N + pad, p["dD"], N + pad,
                                                     tc.cuda.current_stream().cuda_stream)
        tc.cuda.synchronize()
        out = {k: x.cpu().numpy() for k, x in buf.items()}
        out["dS"], out["dD"] = out["dS"][:self.nnz], out["dD"][:self.nnz]
        return out


_refs = {}


def inputs(N):
    """the 400 x 300 matrix of the reduce tests (empty rows, one row of 300) with V, D and G uniform in +-1 and S in +-4"""
    rp, ci, v, M, K, V, D, G = es.inputs(N)
    return rp, ci, v, M, K, scores(1000 + N, len(ci), N), V, D, G


def base_case(mode, N):
    """inputs(N) and the float64 reference, computed once per case"""
    key = (mode, N)
    if key not in _refs:
        rp, ci, v, M, K, S, V, D, G = inputs(N)
        _refs[key] = (rp, ci, v, M, K, S, V, D, G, reference(mode, rp, ci, S, V, D, G, K))
    return _refs[key]


def check(mode, got_fwd, got_bwd, want, tag=""):
    """C, lse and the mode's gradients under _close, each error / limit printed first"""
    wC, wL, wdS, wdV, wdD = want
    C, lse = got_fwd
    print(mode, tag, "C error / limit", limit_ratio(C, wC), "lse", limit_ratio(lse, wL))
    assert _close(C, wC) and lse_close(lse, wL)
    for name, w in (("dS", wdS), ("dV", wdV), ("dD", wdD)):
        if name in grads_of(mode):
            print(mode, tag, name, "error / limit", limit_ratio(got_bwd[name], w), "of max |ref|", float(np.abs(w).max()))
            assert _close(got_bwd[name], w), name


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("mode", list(MODES))
def test_tolerance_pass_selection_and_leading_dimensions(sx, mode, N):
    rp, ci, v, M, K, S, V, D, G, want = base_case(mode, N)
    names = grads_of(mode)
    a = VattAbi(sx, rp, ci, v, M, K)
    C, lse, _, _ = a.fwd(mode, S, V, D)
    assert a.eng.last_kernel() == "vector_attention"
    # dS alone and dD alone need no A^T: none is built
    alone = {name: a.bwd(mode, S, V, D, C, lse, G, want=(name,)) for name in names if name != "dV"}
    assert a.eng.get_stat("transpose_build_s") == 0
    got = a.bwd(mode, S, V, D, C, lse, G, want=names)
    assert a.eng.last_kernel() == "vector_attention_backward"
    if "dV" in names:
        assert a.eng.get_stat("transpose_build_s") > 0
        alone["dV"] = a.bwd(mode, S, V, D, C, lse, G, want=("dV",))
    check(mode, (C, lse), got, want, "N=%d" % N)
    empty = np.flatnonzero(np.diff(rp) == 0)
    assert len(empty) > 10
    assert np.all(C[empty].view(np.uint32) == 0) and np.all(lse[empty] == -np.inf)
    # every subset of the gradients: the same bits, the others' buffers untouched
    for name in names:
        assert same(alone[name][name], got[name]), name
        for other in GRADS:
            if other != name:
                assert np.all(alone[name][other] == 7.0), (name, other)
    if len(names) == 3:
        for left_out in names:
            pair = [g for g in names if g != left_out]
            two = a.bwd(mode, S, V, D, C, lse, G, want=pair)
            assert all(same(two[g], got[g]) for g in pair) and np.all(two[left_out] == 7.0), left_out
    # no gradient at all, and one of an operand the mode does not read: refused
    with pytest.raises(sx.SextansError):
        a.bwd(mode, S, V, D, C, lse, G, want=())
    for name in GRADS:
        if name not in names:
            with pytest.raises(sx.SextansError):
                a.bwd(mode, S, V, D, C, lse, G, want=("dS", name))
    # the operand the mode does not read is ignored: absent, the same bits
    if mode != "add":
        C2, lse2, _, _ = a.fwd(mode, S, V if mode == "node" else None, D if mode == "edge" else None)
        assert same(C2, C) and same(lse2, lse)
    # leading dimensions beyond N: the same bits written in place, the columns beyond N left alone; no lse
    C2, lse2, Cb, Lb = a.fwd(mode, S, V, D, pad=(4, 8, 12, 16, 20))
    assert same(C2, C) and same(lse2, lse)
    assert np.all(Cb[:, N:] == POISON) and np.all(Lb[:, N:] == POISON)
    C2, _, _, Lb = a.fwd(mode, S, V, D, want_lse=False)
    assert same(C2, C) and np.all(Lb == POISON)
    wide = a.bwd(mode, S, V, D, C, lse, G, want=names, pad=12)
    for name in GRADS:
        if name in names:
            assert same(wide[name][:, :N], got[name]) and np.all(wide[name][:, N:] == 7.0), name
        else:
            assert np.all(wide[name] == 7.0), name
    a.eng.close()


@pytest.mark.parametrize("N", [8, 16, 24, 64])
def test_scores_formed_from_the_messages_give_the_parents_bits(sx, N):
    """S = t[n] m_e formed on the host as ONE rounded fp32 product: ADD returns the bits of spmm_edge_softagg ADD, EDGE those of its COPY,
    NODE those of spmm_softagg on an engine whose values are all 1 -- the same online softmax, the same 4 entries in flight, the same
    tiles up to N = 64"""
    rp, ci, v, M, K, _, V, D, G = inputs(N)
    t = temps(N)
    ones = np.ones(len(ci), np.float32)
    a = VattAbi(sx, rp, ci, ones, M, K)
    got = {}
    for mode in MODES:
        m = messages32(mode, V, D, ci)
        S = t[None, :] * m
        assert S.dtype == np.float32
        got[mode] = a.fwd(mode, S, V, D)[:2]
    a.eng.close()
    p = es.EdgeSoftAbi(sx, rp, ci, ones, M, K)
    want = {"add": p.fwd("add", V, D, t)[:2], "edge": p.fwd("copy", None, D, t)[:2]}
    p.eng.close()
    s = SoftAbi(sx, rp, ci, ones, M, K)
    want["node"] = s.fwd(V, t)[:2]
    s.eng.close()
    for mode in MODES:
        assert np.any(got[mode][0] != 0)
        assert bits_equal(got[mode][0], want[mode][0]) and bits_equal(got[mode][1], want[mode][1]), mode


@pytest.mark.parametrize("mode", list(MODES))
def test_rows_of_one_entry(sx, mode):
    """every eighth row cut down to its first entry: w = 1, z = 1, C has the message's bits (+0 for -0) and lse = s"""
    N = 24
    rp, ci, v, M, K, S, V, D, G = inputs(N)
    kept = np.arange(len(ci))
    rp1, ci1, kept = cut_rows(rp, ci, kept)
    S1, D1 = S[kept], D[kept]
    single = np.flatnonzero(np.diff(rp1) == 1)
    assert len(single) >= 40
    a = VattAbi(sx, rp1, ci1, v[kept], M, K)
    C, lse, _, _ = a.fwd(mode, S1, V, D1)
    a.eng.close()
    w1 = reference(mode, rp1, ci1, S1, V, D1)
    assert _close(C, w1[0]) and lse_close(lse, w1[1])
    m1 = messages32(mode, V, D1, ci1)[rp1[single]]
    assert np.any(m1 != 0) and bits_equal(C[single], m1 + np.float32(0))
    assert bits_equal(lse[single], S1[rp1[single]])


@pytest.mark.parametrize("mode", list(MODES))
def test_a_third_of_the_scores_masked(sx, mode):
    """-inf at a random third of the (entry, column) pairs: their weight is +0 and dS is +0 (the bits); everything else agrees with the
    reference, in which exp(-inf) removes those entries"""
    N = 24
    rp, ci, v, M, K, S, V, D, G = inputs(N)
    rs = np.random.RandomState(31)
    mask = rs.rand(*S.shape) < 1.0 / 3
    # no (row, column) fully masked here: the first entry of every row stays
    mask[rp[:-1][np.diff(rp) > 0]] = False
    S2 = S.copy()
    S2[mask] = -np.inf
    want = reference(mode, rp, ci, S2, V, D, G, K)
    assert np.all(np.isfinite(want[0]))
    a = VattAbi(sx, rp, ci, v, M, K)
    C, lse, _, _ = a.fwd(mode, S2, V, D)
    got = a.bwd(mode, S2, V, D, C, lse, G, want=grads_of(mode))
    a.eng.close()
    check(mode, (C, lse), got, want, "masked")
    assert mask.sum() > 1000 and np.all(got["dS"][mask].view(np.uint32) == 0)
    if mode != "node":   # dD is G w: a weight of exactly +0
        assert np.all(got["dD"][mask] == 0)
        assert np.all(got["dD"][mask & (G[rows_of(rp)] > 0)].view(np.uint32) == 0)


def test_one_row_and_column_fully_masked(sx):
    """all scores of one (row, column) -inf: 0 / 0, NaN in C there and nowhere else; lse is -inf there"""
    N, mode = 24, "add"
    rp, ci, v, M, K, S, V, D, G = inputs(N)
    r0 = int(np.flatnonzero(np.diff(rp) == 300)[0])
    n0 = 19
    S2 = S.copy()
    S2[rp[r0]:rp[r0 + 1], n0] = -np.inf
    a = VattAbi(sx, rp, ci, v, M, K)
    C, lse, _, _ = a.fwd(mode, S, V, D)
    C2, lse2, _, _ = a.fwd(mode, S2, V, D)
    a.eng.close()
    hit = np.zeros((M, N), bool)
    hit[r0, n0] = True
    assert np.array_equal(np.isnan(C2), hit) and lse2[r0, n0] == -np.inf
    assert same(C2[~hit], C[~hit]) and same(lse2[~hit], lse[~hit])


@pytest.mark.parametrize("mode", list(MODES))
def test_whole_partial_states_of_a_long_row_masked(sx, mode):
    """the 2500-entry row of pattern P with its first 1024 scores -inf in every column: every slot of the long-row kernel's workgroup
    starts on -inf only, and whole partial states of narrower dealings hold nothing else; the row stays finite and within tolerance"""
    N, p = 16, pat("P")
    r0 = int(np.flatnonzero(p.lens == 2500)[0])
    rs = np.random.RandomState(5)
    half = np.float32(0.5)
    S, V, D, G = scores(6, p.nnz, N), rand(rs, p.K, N) * half, rand(rs, p.nnz, N) * half, rand(rs, p.M, N)
    S[p.rp[r0]:p.rp[r0] + 1024] = -np.inf
    want = reference(mode, p.rp, p.ci, S, V, D, G, p.K)
    a = VattAbi(sx, p.rp, p.ci, np.ones(p.nnz, np.float32), p.M, p.K)
    C, lse, _, _ = a.fwd(mode, S, V, D)
    assert a.eng.last_kernel() == "vector_attention+long_rows"
    got = a.bwd(mode, S, V, D, C, lse, G, want=grads_of(mode))
    a.eng.close()
    assert np.all(np.isfinite(C)) and np.all(np.isfinite(lse[p.ne]))
    check(mode, (C, lse), got, want, "long row")
    assert np.all(got["dS"][p.rp[r0]:p.rp[r0] + 1024].view(np.uint32) == 0)


def test_degenerate_matrices(sx):
    """M == 0 and nnz == 0: OK, C and dV zeroed, lse = -inf; dS and dD have no element"""
    N = 16
    rs = np.random.RandomState(4)
    for M, K in ((0, 7), (9, 7)):
        rp, ci, v = np.zeros(M + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)
        S, V, D, G = np.zeros((0, N), np.float32), rand(rs, K, N), np.zeros((0, N), np.float32), rand(rs, M, N)
        a = VattAbi(sx, rp, ci, v, M, K)
        for mode in MODES:
            C, lse, _, _ = a.fwd(mode, S, V, D)
            assert C.shape == (M, N) and np.all(C.view(np.uint32) == 0) and np.all(lse == -np.inf)
            got = a.bwd(mode, S, V, D, C, lse, G, want=grads_of(mode))
            if mode != "edge":
                assert np.all(got["dV"].view(np.uint32) == 0), mode
            assert got["dS"].shape == (0, N) and got["dD"].shape == (0, N)
        a.eng.close()


def test_determinism_streams_and_graph_replay(sx):
    import torch
    N, mode = 24, "add"
    rp, ci, v, M, K, S, V, D, G = inputs(N)
    a = VattAbi(sx, rp, ci, v, M, K)

    def both():
        C, lse, _, _ = a.fwd(mode, S, V, D)
        g = a.bwd(mode, S, V, D, C, lse, G)
        return [C, lse, g["dS"], g["dV"], g["dD"]]

    first, second = both(), both()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = both()
    torch.cuda.current_stream().wait_stream(side)
    for i, (x, y, z) in enumerate(zip(first, second, third)):
        assert same(x, y) and same(x, z), i

    # forward and backward captured once on a single stream (tables and A^T exist: the calls above were the warm-up), replayed once
    St, Vt, Dt, Gt = a.dev(S), a.dev(V), a.dev(D), a.dev(G)
    Ct, Lt = torch.zeros((M, N), device="cuda"), torch.zeros((M, N), device="cuda")
    dS, dV, dD = torch.zeros((a.nnz, N), device="cuda"), torch.zeros((K, N), device="cuda"), torch.zeros((a.nnz, N), device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        s = torch.cuda.current_stream().cuda_stream
        a.eng.vector_attention_device_rm(MODES[mode], N, St.data_ptr(), N, Vt.data_ptr(), N, Dt.data_ptr(), N, Ct.data_ptr(), N,
                                         Lt.data_ptr(), N, s)
        a.eng.vector_attention_backward_device_rm(MODES[mode], N, St.data_ptr(), N, Vt.data_ptr(), N, Dt.data_ptr(), N, Ct.data_ptr(), N,
                                                  Lt.data_ptr(), N, Gt.data_ptr(), N, dS.data_ptr(), N, dV.data_ptr(), N, dD.data_ptr(), N, s)
    g.replay()
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip((Ct, Lt, dS, dV, dD), first)):
        assert same(x.cpu().numpy(), y), i
    a.eng.close()
