"""Softmax aggregation of edge-feature messages on the GPU (sextans_spmm_edge_softagg_device_rm / _backward_device_rm,
edge_softagg.spmm_edge_softagg): C, lse, dB, dE and dt against a float64 numpy reference built row by row from the fp32-rounded
messages; exact bits where the arithmetic fixes them (empty rows, rows of one entry, COPY fed another op's messages against that op,
MUL fed E[e, :] = val[e] against spmm_softagg); overflow safety at |t| = 200; a NaN stays in its (row, column); degenerate matrices;
determinism across runs, streams and graph replay; the torch op with autograd in B, E and t.

Tolerance: test_torch_autograd_gpu._close (rtol 2e-4), the project's tolerance for fp32 sums.  ADD messages reach |m| = 2 where
spmm_softagg's products stay below 1, so t (m - C) is larger than in that family's tests.  emulate() below restates the kernels' fp32
arithmetic on the CPU (one entry after the other) and tests/test_spmm_edge_softagg_tolerance.py (no GPU) holds it against the reference
on this module's inputs at the temperatures TEMPS, N = 16.  Largest error / limit over C, lse, dB, dE, dt per op, with B and E uniform
in +-1:
    mul 0.12 (dB)    add 0.17 (dE)    add_relu 0.24 (dE)    copy 0.06 (dE)        (C <= 0.03, lse <= 0.003, dt <= 0.07 everywhere)
-- all below 0.5, so no op's inputs are shrunk.  Gradients are not compared at |t| >= 100, as in test_spmm_softagg_gpu."""
import numpy as np
import pytest

from test_fused_attention_gpu import rand, same
from test_spmm_edge_gpu import OPS, messages
from test_spmm_reduce_gpu import POISON, Abi, base_matrix, bits_equal
from test_spmm_softagg_gpu import HOT, TEMPS, SoftAbi, cut_rows, lse_close, temps
from test_torch_attention_gpu import make_A
from test_torch_autograd_gpu import _close

pytestmark = pytest.mark.gpu

GRADS = ("dB", "dE", "dt")


def rows_of(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


def messages32(op, B, E, ci):
    """(nnz, N) float32: the kernels' messages, one rounded operation each"""
    m = messages(op, B[ci].astype(np.float32) if op != "copy" else None, E.astype(np.float32))
    assert m.dtype == np.float32
    return m


def reference(op, rp, ci, B, E, t, G=None, K=None):
    """float64, row by row, from the fp32-rounded messages: (C, lse) or, with G, (C, lse, dB, dE, dt); dB None for copy.  t None = 1."""
    M, N = len(rp) - 1, E.shape[1]
    t64 = np.ones(N) if t is None else t.astype(np.float64)
    m = messages32(op, B, E, ci).astype(np.float64)
    C, lse = np.zeros((M, N)), np.full((M, N), -np.inf)
    q = np.zeros_like(m)
    dt = np.zeros(N)
    with np.errstate(invalid="ignore"):
        for r in range(M):
            b, e = rp[r], rp[r + 1]
            if e == b:
                continue
            P = m[b:e]
            s = t64 * P
            mx = s.max(0)
            w = np.exp(s - mx)
            z = w.sum(0)
            w /= z
            C[r] = (w * P).sum(0)
            lse[r] = mx + np.log(z)
            if G is not None:
                d = P - C[r]
                q[b:e] = G[r].astype(np.float64) * w * (1 + t64 * d)
                dt += G[r].astype(np.float64) * (w * P * d).sum(0)
    if G is None:
        return C, lse
    E64 = E.astype(np.float64)
    if op == "mul":
        dE, tB = q * B.astype(np.float64)[ci], q * E64
    elif op == "add_relu":
        dE = tB = np.where(B.astype(np.float32)[ci] + E.astype(np.float32) > 0, q, 0.0)
    else:
        dE = tB = q
    dB = None
    if op != "copy":
        dB = np.zeros((K, N))
        np.add.at(dB, ci, tB)
    return C, lse, dB, dE, dt


def emulate(op, rp, ci, B, E, t, G, K, slots=1):
    """The kernels' arithmetic in float32 on the CPU: (C, lse, dB, dE, dt).  One entry order: a row's entries one after the other
    (slots = 1) or, for a row of at least 2 * slots entries, dealt to `slots` partial states (entry k to state k % slots, as
    pattern_pass.h deals a row to its slots), which a pairwise tree then merges with the kernels' combine; dt's row sums likewise.  dB adds
    a column's entries one after the other.  fma is one rounding of the float64 expression; exp and log are numpy's float32 ones."""
    f32, f64 = np.float32, np.float64
    M, N = len(rp) - 1, E.shape[1]
    fma = lambda x, y, z: (x.astype(f64) * y.astype(f64) + np.asarray(z, f64)).astype(f32)   # noqa: E731
    m = messages32(op, B, E, ci)
    s = m if t is None else (t[None, :] * m).astype(f32)
    C, lse = np.zeros((M, N), f32), np.full((M, N), -np.inf, f32)

    def dealt(b, e):
        """-> (S, steps, the (steps, S) entry positions, their validity)"""
        S = slots if e - b >= 2 * slots else 1
        steps = -(-(e - b) // S)
        pos = b + np.arange(steps * S).reshape(steps, S)
        return S, steps, np.minimum(pos, e - 1), pos < e

    with np.errstate(all="ignore"):
        for r in range(M):
            if rp[r + 1] == rp[r]:
                continue
            S, steps, pos, ok = dealt(rp[r], rp[r + 1])
            mx, z, acc = np.full((S, N), -np.inf, f32), np.zeros((S, N), f32), np.zeros((S, N), f32)
            for k in range(steps):
                sk, mk = np.where(ok[k][:, None], s[pos[k]], f32(-np.inf)), m[pos[k]]
                mn = np.maximum(mx, sk)
                ref = np.where(mn == -np.inf, f32(0), mn)
                al, w = np.exp(mx - ref), np.exp(sk - ref)
                z, acc, mx = z * al + w, fma(w, mk, acc * al), mn
            while S > 1:   # the tree: state j with state j + S / 2
                S //= 2
                mn = np.maximum(mx[:S], mx[S:])
                ref = np.where(mn == -np.inf, f32(0), mn)
                ca, cb = np.exp(mx[:S] - ref), np.exp(mx[S:] - ref)
                z, acc, mx = z[:S] * ca + z[S:] * cb, acc[:S] * ca + acc[S:] * cb, mn
            C[r], lse[r] = acc[0] / z[0], mx[0] + np.log(z[0])
        rows = rows_of(rp)
        w = np.exp(s - lse[rows])
        d = m - C[rows]
        gw = G[rows] * w
        q = gw * (fma(t[None, :] * np.ones_like(d), d, 1.0) if t is not None else d + f32(1))
        assert q.dtype == f32
        zero = np.zeros_like(q)
        Bc = B[ci] if op != "copy" else None
        if op == "mul":
            dE, tB = q * Bc, q * E
        elif op == "add_relu":
            dE = tB = np.where(Bc + E > 0, q, zero)
        else:
            dE = tB = q
        dB = None
        if op != "copy":
            dB = np.zeros((K, N), f32)
            np.add.at(dB, ci, tB)          # (float32 adds, in entry order)
        dt_rows = np.zeros((M, N), f32)
        terms = gw * (m * d)
        for r in range(M):
            if rp[r + 1] == rp[r]:
                continue
            S, steps, pos, ok = dealt(rp[r], rp[r + 1])
            part = np.zeros((S, N), f32)
            for k in range(steps):
                part = part + np.where(ok[k][:, None], terms[pos[k]], f32(0))
            while S > 1:
                S //= 2
                part = part[:S] + part[S:]
            dt_rows[r] = part[0]
        dt = np.zeros(N, f32)
        for r in range(M):
            dt = dt + dt_rows[r]
    return C, lse, dB, dE, dt


def limit_ratio(got, want):
    """the largest |got - want| / limit of _close; lse: over the finite entries"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    lim = 2e-4 * (np.abs(want[fin]) + np.abs(want[fin]).max() * 1e-2)
    return float((np.abs(got[fin] - want[fin]) / lim).max())


class EdgeSoftAbi(Abi):
    """test_spmm_reduce_gpu.Abi's engine on a matrix, the edge-feature softmax aggregation's entry points called through api.Engine"""

    def fwd(self, op, B, E, t=None, want_lse=True, pad=(0, 0, 0, 0), stream=None):
        """-> (C, lse) as numpy and the whole padded buffers as int32; pad: extra columns of the B / E / C / lse buffers"""
        tc = self.t
        N = E.shape[1]
        Bb = None
        if op != "copy":
            Bb = tc.zeros((self.K, N + pad[0]), device="cuda")
            Bb[:, :N] = tc.from_numpy(B)
        Eb = tc.zeros((max(self.nnz, 1), N + pad[1]), device="cuda")
        Eb[:self.nnz, :N] = tc.from_numpy(E)
        Cb = tc.full((max(self.M, 1), N + pad[2]), POISON, dtype=tc.int32, device="cuda")
        Lb = tc.full((max(self.M, 1), N + pad[3]), POISON, dtype=tc.int32, device="cuda")
        tt = tc.from_numpy(t).cuda() if t is not None else None
        self.eng.spmm_edge_softagg_device_rm(OPS[op], N, Bb.data_ptr() if Bb is not None else None, N + pad[0], Eb.data_ptr(), N + pad[1],
                                             tt.data_ptr() if tt is not None else None, Cb.data_ptr(), N + pad[2],
                                             Lb.data_ptr() if want_lse else None, N + pad[3], tc.cuda.current_stream().cuda_stream)
        tc.cuda.synchronize()
        Cn, Ln = Cb.cpu().numpy()[:self.M], Lb.cpu().numpy()[:self.M]
        return Cn[:, :N].view(np.float32), Ln[:, :N].view(np.float32), Cn, Ln

    def bwd(self, op, B, E, t, C, lse, G, want=GRADS, work=True):
        """-> {name: numpy} of the three gradients and the workspace: the ones not in `want` get no pointer and must keep their 7.0"""
        tc = self.t
        N = G.shape[1]
        dev = lambda x: tc.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
        Et, Ct, Lt, Gt = (dev(x) for x in (E, C, lse, G))
        Bt = dev(B) if op != "copy" else None
        tt = dev(t) if t is not None else None
        nwork = self.eng.spmm_edge_softagg_workspace_floats(N)
        assert nwork == self.M * N + (self.M + 255) // 256 * N
        buf = {"dB": tc.full((self.K, N), 7.0, device="cuda"), "dE": tc.full((max(self.nnz, 1), N), 7.0, device="cuda"),
               "dt": tc.full((N,), 7.0, device="cuda"), "work": tc.full((max(nwork, 1),), 7.0, device="cuda")}
        p = {k: (x.data_ptr() if k in want or (k == "work" and work) else None) for k, x in buf.items()}
        ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None   # noqa: E731
        self.eng.spmm_edge_softagg_backward_device_rm(OPS[op], N, ptr(Bt), N, ptr(Et), N, ptr(tt), ptr(Ct), N, ptr(Lt), N, ptr(Gt), N,
                                                      p["dB"], N, p["dE"], N, p["dt"], p["work"], tc.cuda.current_stream().cuda_stream)
        tc.cuda.synchronize()
        out = {k: x.cpu().numpy() for k, x in buf.items()}
        out["dE"] = out["dE"][:self.nnz]
        return out


_refs = {}


def inputs(N):
    """the 400 x 300 matrix of the reduce tests (empty rows, one row of 300) with B, E and G uniform in +-1"""
    rs, rp, ci, v, M, K = base_matrix(5)
    return rp, ci, v, M, K, rand(rs, K, N), rand(rs, len(ci), N), rand(rs, M, N)


def base_case(op, N, cycle="temps"):
    """inputs(N), t and the float64 reference, computed once per case"""
    key = (op, N, cycle)
    if key not in _refs:
        rp, ci, v, M, K, B, E, G = inputs(N)
        t = {"temps": temps(N), "hot": temps(N, HOT), "none": None}[cycle]
        _refs[key] = (rp, ci, v, M, K, B, E, G, t, reference(op, rp, ci, B, E, t, G, K))
    return _refs[key]


@pytest.mark.parametrize("cycle", ["none", "temps"])
@pytest.mark.parametrize("N", [8, 16, 24, 64, 136])
@pytest.mark.parametrize("op", list(OPS))
def test_forward_on_the_c_abi(sx, op, N, cycle):
    """one tile, a partial tile (24), three tiles with a partial last one (136); d_t NULL and per-column temperatures; padded leading
    dimensions with the padding left alone; no lse; the exact bits of empty rows and of rows of one entry"""
    rp, ci, v, M, K, B, E, G, t, (wC, wL, _, _, _) = base_case(op, N, cycle)
    a = EdgeSoftAbi(sx, rp, ci, v, M, K)
    C, lse, _, _ = a.fwd(op, B, E, t)
    assert a.eng.last_kernel() == "spmm_edge_softagg"
    print(op, N, cycle, "C error / limit", limit_ratio(C, wC), "lse error / limit", limit_ratio(lse, wL))
    assert _close(C, wC) and lse_close(lse, wL)
    empty = np.flatnonzero(np.diff(rp) == 0)
    assert len(empty) > 10
    assert np.all(C[empty].view(np.uint32) == 0) and np.all(lse[empty] == -np.inf)
    C2, lse2, Cb, Lb = a.fwd(op, B, E, t, pad=(4, 8, 12, 16))
    assert same(C2, C) and same(lse2, lse)
    assert np.all(Cb[:, N:] == POISON) and np.all(Lb[:, N:] == POISON)
    C2, _, _, Lb = a.fwd(op, B, E, t, want_lse=False)
    assert same(C2, C) and np.all(Lb == POISON)
    a.eng.close()
    # rows of one entry (the matrix above has none: every eighth row cut down to its first entry): w = 1, z = 1, C has the message's bits
    rp1, ci1, kept = cut_rows(rp, ci, np.arange(len(ci)))
    E1 = E[kept]
    single = np.flatnonzero(np.diff(rp1) == 1)
    assert len(single) >= 40
    a = EdgeSoftAbi(sx, rp1, ci1, v[kept], M, K)
    C, lse, _, _ = a.fwd(op, B, E1, t)
    a.eng.close()
    w1 = reference(op, rp1, ci1, B, E1, t)
    assert _close(C, w1[0]) and lse_close(lse, w1[1])
    m1 = messages32(op, B, E1, ci1)[rp1[single]]
    assert np.any(m1 != 0) and bits_equal(C[single], m1 + np.float32(0))   # (a -0 message gives +0; add_relu has +0 messages)


@pytest.mark.parametrize("cycle", ["none", "temps"])
@pytest.mark.parametrize("N", [16, 136])
@pytest.mark.parametrize("op", ["mul", "add", "add_relu"])
def test_copy_of_the_messages_has_the_ops_bits(sx, op, N, cycle):
    """(a) COPY fed E := m_op (numpy float32) returns the bits of C and lse of the op's own forward: a wrong operand or tile shows"""
    rp, ci, v, M, K, B, E, G, t, _ = base_case(op, N, cycle)
    a = EdgeSoftAbi(sx, rp, ci, v, M, K)
    C, lse, _, _ = a.fwd(op, B, E, t)
    Cc, lsec, _, _ = a.fwd("copy", None, messages32(op, B, E, ci), t)
    a.eng.close()
    assert bits_equal(Cc, C) and bits_equal(lsec, lse)


@pytest.mark.parametrize("cycle", ["none", "temps"])
@pytest.mark.parametrize("N", [8, 16, 24, 64])
def test_mul_of_broadcast_values_is_spmm_softagg(sx, N, cycle):
    """(b) MUL with E[e, :] = val[e] returns the BITS of sextans_spmm_softagg_device_rm(val, B, t) -- the same online softmax, the same
    entries in flight, the same tiles up to N = 64; (c) the row sums of dE agree with that family's dval"""
    rp, ci, v, M, K, B, _, G, t, _ = base_case("mul", N, cycle)
    E = np.repeat(v[:, None], N, 1).astype(np.float32)
    a = EdgeSoftAbi(sx, rp, ci, v, M, K)
    C, lse, _, _ = a.fwd("mul", B, E, t)
    got = a.bwd("mul", B, E, t, C, lse, G)
    a.eng.close()
    s = SoftAbi(sx, rp, ci, v, M, K)
    Cs, lses, _, _ = s.fwd(B, t)
    gs = s.bwd(B, t, Cs, lses, G)
    s.eng.close()
    assert bits_equal(C, Cs) and bits_equal(lse, lses)
    assert _close(got["dE"].astype(np.float64).sum(1), gs["dval"])
    assert _close(got["dB"], gs["dB"]) and _close(got["dt"], gs["dt"])


@pytest.mark.parametrize("N", [8, 24, 64, 136])
@pytest.mark.parametrize("op", list(OPS))
def test_backward_on_the_c_abi(sx, op, N):
    rp, ci, v, M, K, B, E, G, t, (wC, wL, wdB, wdE, wdt) = base_case(op, N)
    names = [g for g in GRADS if not (op == "copy" and g == "dB")]
    a = EdgeSoftAbi(sx, rp, ci, v, M, K)
    C, lse, _, _ = a.fwd(op, B, E, t)
    # dt alone and dE alone need no A^T: none is built
    alone = {name: a.bwd(op, B, E, t, C, lse, G, want=(name,)) for name in ("dt", "dE")}
    assert a.eng.get_stat("transpose_build_s") == 0
    got = a.bwd(op, B, E, t, C, lse, G, want=names)
    assert a.eng.last_kernel() == "spmm_edge_softagg_backward"
    if op != "copy":
        assert a.eng.get_stat("transpose_build_s") > 0
        alone["dB"] = a.bwd(op, B, E, t, C, lse, G, want=("dB",))
    for name, want in (("dB", wdB), ("dE", wdE), ("dt", wdt)):
        if name in names:
            print(op, N, name, "error / limit", limit_ratio(got[name], want), "of max |ref|", float(np.abs(want).max()))
            assert _close(got[name], want), name
    # the workspace holds the rows' shares of dt, then the chunk sums
    rows = got["work"][:M * N].reshape(M, N).astype(np.float64)
    assert _close(rows.sum(0), wdt) and np.all(rows[np.diff(rp) == 0] == 0)
    # every subset of the gradients: the same bits, the others' buffers untouched; without dt the workspace is not written either
    for name in names:
        assert same(alone[name][name], got[name]), name
        for other in GRADS:
            if other != name:
                assert np.all(alone[name][other] == 7.0), (name, other)
        assert same(alone[name]["work"], got["work"]) if name == "dt" else np.all(alone[name]["work"] == 7.0), name
    for left_out in names:
        pair = [g for g in names if g != left_out]
        two = a.bwd(op, B, E, t, C, lse, G, want=pair, work="dt" in pair)
        assert all(same(two[g], got[g]) for g in pair) and np.all(two[left_out] == 7.0), left_out
    # d_t NULL is t = 1
    one = np.ones(N, np.float32)
    ones = a.bwd(op, B, E, one, *a.fwd(op, B, E, one)[:2], G, want=names)
    null = a.bwd(op, B, E, None, *a.fwd(op, B, E, None)[:2], G, want=names)
    for name in names:
        assert _close(null[name], ones[name]), name
    if op == "copy":   # COPY has no dB: asking for it is refused
        with pytest.raises(sx.SextansError):
            a.bwd(op, B, E, t, C, lse, G, want=("dB", "dE"))
    a.eng.close()


@pytest.mark.parametrize("op", list(OPS))
def test_overflow_safety_forward(sx, op):
    """t m far beyond +-88: only differences to the running maximum are exponentiated"""
    N = 16
    rp, ci, v, M, K, B, E, G, t, (wC, wL, _, _, _) = base_case(op, N, "hot")
    assert np.abs(t[None, :] * messages32(op, B, E, ci)).max() > 150
    a = EdgeSoftAbi(sx, rp, ci, v, M, K)
    C, lse, _, _ = a.fwd(op, B, E, t)
    a.eng.close()
    full = np.diff(rp) > 0
    assert np.all(np.isfinite(C)) and np.all(np.isfinite(lse[full]))
    print(op, "C error / limit", limit_ratio(C, wC), "lse error / limit", limit_ratio(lse, wL))
    assert _close(C, wC) and lse_close(lse, wL)


@pytest.mark.parametrize("op", list(OPS))
def test_a_nan_stays_in_its_row_and_column(sx, op):
    N = 24
    rp, ci, v, M, K, B, E, G, t, _ = base_case(op, N)
    r0 = int(np.flatnonzero(np.diff(rp) == 300)[0])
    e0, n0 = int(rp[r0]) + 170, 19
    E2 = E.copy()
    E2[e0, n0] = np.nan
    a = EdgeSoftAbi(sx, rp, ci, v, M, K)
    C, lse, _, _ = a.fwd(op, B, E, t)
    C2, lse2, _, _ = a.fwd(op, B, E2, t)
    a.eng.close()
    hit = np.zeros((M, N), bool)
    hit[r0, n0] = True
    assert np.array_equal(np.isnan(C2), hit) and np.array_equal(np.isnan(lse2), hit)
    assert same(C2[~hit], C[~hit]) and same(lse2[~hit], lse[~hit])


def test_degenerate_matrices(sx):
    """M == 0 and nnz == 0: OK, the outputs zeroed, lse = -inf, the gradients zeroed"""
    N = 16
    rs = np.random.RandomState(4)
    for M, K in ((0, 7), (9, 7)):
        rp, ci, v = np.zeros(M + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)
        B, E, G = rand(rs, K, N), np.zeros((0, N), np.float32), rand(rs, M, N)
        a = EdgeSoftAbi(sx, rp, ci, v, M, K)
        for op in OPS:
            C, lse, _, _ = a.fwd(op, B, E, temps(N))
            assert C.shape == (M, N) and np.all(C.view(np.uint32) == 0) and np.all(lse == -np.inf)
            names = [g for g in GRADS if not (op == "copy" and g == "dB")]
            got = a.bwd(op, B, E, temps(N), C, lse, G, want=names)
            for name in names:
                assert np.all(got[name] == 0), (op, name)
            assert np.all(got["work"][:M * N + (M + 255) // 256 * N] == 0)
        a.eng.close()


def test_determinism_streams_and_graph_replay(sx):
    import torch
    N, op = 24, "add_relu"
    rp, ci, v, M, K, B, E, G, t, _ = base_case(op, N)
    rs = np.random.RandomState(77)
    G2, E2 = rand(rs, M, N), rand(rs, len(ci), N)
    a = EdgeSoftAbi(sx, rp, ci, v, M, K)

    def both(En, Gn):
        C, lse, _, _ = a.fwd(op, B, En, t)
        g = a.bwd(op, B, En, t, C, lse, Gn)
        return [C, lse, g["dB"], g["dE"], g["dt"]]

    first, second = both(E, G), both(E, G)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = both(E, G)
    torch.cuda.current_stream().wait_stream(side)
    for i, (x, y, z) in enumerate(zip(first, second, third)):
        assert same(x, y) and same(x, z), i
    want = both(E2, G2)
    assert not same(want[0], first[0]) and not same(want[2], first[2])

    # forward and backward captured on a side stream (tables and A^T exist: the calls above were the warm-up), replayed twice with
    # other operands
    tc = torch
    dev = lambda x: tc.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
    Bt, Et, Gt, tt = dev(B), dev(E), dev(G), dev(t)
    Ct, Lt = tc.zeros((M, N), device="cuda"), tc.zeros((M, N), device="cuda")
    dB, dE, dt = tc.zeros((K, N), device="cuda"), tc.zeros((a.nnz, N), device="cuda"), tc.zeros((N,), device="cuda")
    work = tc.zeros((a.eng.spmm_edge_softagg_workspace_floats(N),), device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        s = torch.cuda.current_stream().cuda_stream
        a.eng.spmm_edge_softagg_device_rm(OPS[op], N, Bt.data_ptr(), N, Et.data_ptr(), N, tt.data_ptr(), Ct.data_ptr(), N, Lt.data_ptr(), N, s)
        a.eng.spmm_edge_softagg_backward_device_rm(OPS[op], N, Bt.data_ptr(), N, Et.data_ptr(), N, tt.data_ptr(), Ct.data_ptr(), N,
                                                   Lt.data_ptr(), N, Gt.data_ptr(), N, dB.data_ptr(), N, dE.data_ptr(), N, dt.data_ptr(),
                                                   work.data_ptr(), s)
    for En, Gn, ref in ((E2, G2, want), (E, G, first)):
        Et.copy_(dev(En)); Gt.copy_(dev(Gn))
        g.replay()
        torch.cuda.synchronize()
        for i, (x, y) in enumerate(zip((Ct, Lt, dB, dE, dt), ref)):
            assert same(x.cpu().numpy(), y), i
    a.eng.close()


# --- torch ---------------------------------------------------------------------------------------------------------------------------
def torch_reference(op, rp, ci, M, K, B, E, t, G, eps=0.0):
    """a float64 composition on the CPU with torch's autograd, the messages materialised: (C, dB or None, dE, dt)"""
    import torch
    rows = torch.from_numpy(rows_of(rp))
    cols = torch.from_numpy(ci.astype(np.int64))
    Bt = torch.from_numpy(B.astype(np.float64)).requires_grad_() if op != "copy" else None
    Et = torch.from_numpy(E.astype(np.float64)).requires_grad_()
    tt = torch.from_numpy(np.broadcast_to(np.asarray(t, np.float64), (E.shape[1],)).copy()).requires_grad_()
    m = {"mul": lambda: Bt[cols] * Et, "add": lambda: Bt[cols] + Et, "add_relu": lambda: torch.relu(Bt[cols] + Et), "copy": lambda: Et * 1}[op]()
    m = m + eps
    s = tt * m
    mx = torch.full((M, E.shape[1]), -np.inf, dtype=torch.float64).scatter_reduce(0, rows[:, None].expand_as(s), s.detach(), "amax")
    w = torch.exp(s - mx[rows])
    z = torch.zeros((M, E.shape[1]), dtype=torch.float64).index_add(0, rows, w)
    C = torch.zeros((M, E.shape[1]), dtype=torch.float64).index_add(0, rows, w / z[rows] * m)
    C.backward(torch.from_numpy(G.astype(np.float64)))
    return C.detach().numpy(), (Bt.grad.numpy() if Bt is not None else None), Et.grad.numpy(), tt.grad.numpy()


@pytest.mark.parametrize("N", [12, 16])
@pytest.mark.parametrize("op", list(OPS))
def test_torch_autograd(sx, op, N):
    """N = 12 (no multiple of 8) through the padded copies; gradients of B, E and an (N,) t against the float64 composition; one engine,
    no value refresh; lse; a zero-stride upstream gradient"""
    import torch
    from sextans_amd import edge_softagg, torch_op
    rp, ci, v, M, K, B, E, G = inputs(N)
    t = temps(N)
    wC, wdB, wdE, wdt = torch_reference(op, rp, ci, M, K, B, E, t, G)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    Bt = torch.from_numpy(B).cuda().requires_grad_() if op != "copy" else None
    Et = torch.from_numpy(E).cuda().requires_grad_()
    tt = torch.from_numpy(t).cuda().requires_grad_()
    out, lse = edge_softagg.spmm_edge_softagg(A, Bt, Et, op=op, t=tt, return_lse=True)
    assert out.requires_grad and not lse.requires_grad and out.shape == (M, N) and lse.shape == (M, N)
    out.backward(torch.from_numpy(G).cuda())
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0 and info["entries"] == 1, info
    got = [("C", out.detach(), wC), ("dE", Et.grad, wdE), ("dt", tt.grad, wdt)] + ([("dB", Bt.grad, wdB)] if op != "copy" else [])
    for name, g, w in got:
        g = g.cpu().numpy()
        assert g.shape == w.shape
        print(op, N, name, "error / limit", limit_ratio(g, w))
        assert _close(g, w), name
    assert lse_close(lse.cpu().numpy(), reference(op, rp, ci, B, E, t)[1])
    # without autograd: the same bits; inference computes no lse unless asked
    with torch.no_grad():
        assert same(edge_softagg.spmm_edge_softagg(A, Bt, Et, op=op, t=tt).cpu().numpy(), out.detach().cpu().numpy())
    # .sum().backward(): an upstream gradient with zero strides
    Et.grad = None
    edge_softagg.spmm_edge_softagg(A, Bt, Et, op=op, t=tt).sum().backward()
    ones = torch_reference(op, rp, ci, M, K, B, E, t, np.ones((M, N), np.float32))
    assert _close(Et.grad.cpu().numpy(), ones[2])
    assert torch_op.cache_info() == info
    torch_op.clear_cache()


def test_torch_temperature_forms_eps_and_errors(sx):
    """t as a float, a 0-d tensor and an (N,) tensor; only the gradients asked for; GENConv's message relu(x_j + e_ij) + eps written out
    in float64; t = 0 is the mean; errors"""
    import torch
    from sextans_amd import edge_softagg, torch_op
    N = 16
    rp, ci, v, M, K, B, E, G = inputs(N)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    Bt, Et, Gt = torch.from_numpy(B).cuda().requires_grad_(), torch.from_numpy(E).cuda().requires_grad_(), torch.from_numpy(G).cuda()
    f = edge_softagg.spmm_edge_softagg
    # a scalar temperature: a 0-d gradient, the sum of the vector one; a Python float is that temperature everywhere
    t0 = torch.tensor(0.75, device="cuda", requires_grad=True)
    out = f(A, Bt, Et, op="add", t=t0)
    out.backward(Gt)
    tv = torch.full((N,), 0.75, device="cuda", requires_grad=True)
    outv = f(A, Bt, Et, op="add", t=tv)
    outv.backward(Gt)
    assert same(out.detach().cpu().numpy(), outv.detach().cpu().numpy())
    assert t0.grad.shape == () and _close(t0.grad.cpu().numpy(), tv.grad.sum().cpu().numpy())
    assert same(f(A, Bt.detach(), Et.detach(), op="add", t=0.75).cpu().numpy(), out.detach().cpu().numpy())
    wC, wdB, wdE, wdt = torch_reference("add", rp, ci, M, K, B, E, 0.75, G)
    assert _close(out.detach().cpu().numpy(), wC) and _close(tv.grad.cpu().numpy(), wdt)
    # t = 1.0 is the kernels' d_t == NULL path; B alone wants a gradient
    Bt.grad = Et.grad = None
    f(A, Bt, Et.detach(), op="mul").backward(Gt)
    w1 = torch_reference("mul", rp, ci, M, K, B, E, 1.0, G)
    assert Et.grad is None and _close(Bt.grad.cpu().numpy(), w1[1])
    # GENConv (PyG): message relu(x_j + e_ij) + eps, softmax aggregation with temperature t; empty rows stay 0
    eps, tg = 1e-7, temps(N)
    wC = torch_reference("add_relu", rp, ci, M, K, B, E, tg, G, eps=eps)[0]
    C = f(A, Bt.detach(), Et.detach(), op="add_relu", t=torch.from_numpy(tg).cuda(), eps=eps).cpu().numpy()
    empty = np.diff(rp) == 0
    assert _close(C, wC) and np.all(C[empty] == 0) and np.all(wC[empty] == 0)
    plain = f(A, Bt.detach(), Et.detach(), op="add_relu", t=torch.from_numpy(tg).cuda()).cpu().numpy()
    assert same(C[~empty], plain[~empty] + np.float32(eps))
    # t = 0: the mean of the messages
    for op in OPS:
        Bo = Bt.detach() if op != "copy" else None
        mean = torch_op.spmm_edge(A, Bo, Et.detach(), op=op, reduce="mean").cpu().numpy()
        assert _close(f(A, Bo, Et.detach(), op=op, t=0.0).cpu().numpy(), mean), op
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0, info
    with pytest.raises(ValueError):
        f(A, Bt.detach(), Et.detach(), op="sub")
    with pytest.raises(ValueError):
        f(A, None, Et.detach(), op="mul")
    with pytest.raises(ValueError):
        f(A, Bt.detach(), Et.detach(), op="copy")
    with pytest.raises(TypeError):
        f(A, Bt.detach().cpu(), Et.detach())
    with pytest.raises(ValueError):
        f(A, Bt.detach(), Et.detach()[:-1])
    with pytest.raises(ValueError):
        f(A, Bt.detach(), Et.detach(), t=torch.ones(N + 1, device="cuda"))
    with pytest.raises(TypeError):
        f(A, Bt.detach(), Et.detach(), t=torch.ones(N, device="cuda", dtype=torch.int32))
    torch_op.clear_cache()
