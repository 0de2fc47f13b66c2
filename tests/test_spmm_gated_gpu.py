"""Gated aggregation on the GPU (sextans_spmm_gated_device_rm / _backward_device_rm, sextans_amd.gated.spmm_gated): C, den, z and the
four gradients against a float64 numpy reference built row by row from the fp32 inputs, with a random Gz; exact bits where the
arithmetic fixes them (z, empty rows, saturated gates); padding and optional outputs; long rows; every row-dealing path at one width per
slot shape; determinism across runs, streams and graph replay; the torch op with autograd in all four operands through both outputs.

Tolerance: test_torch_autograd_gpu._close (rtol 2e-4), the project's tolerance for fp32 sums.  A numpy-float32 emulation of the kernels'
arithmetic (compute(..., np.float32): the same expressions, the sums taken sequentially, an unfused multiply-add) on the base case at
N = 16 with operands uniform in (-1, 1) uses at most 0.04 of that limit for any of C, den, z and the four gradients in either mode --
test_emulation_stays_under_half_the_limit (no GPU needed) asserts that it stays under one half."""
import numpy as np
import pytest

from test_fused_attention_gpu import edge_pattern, rand, same
from test_pattern_dealing_gpu import names_ok, pat, rng
from test_spmm_reduce_gpu import POISON, Abi, base_matrix, bits_equal
from test_spmm_softagg_gpu import cut_rows
from test_torch_attention_gpu import make_A
from test_torch_autograd_gpu import _close

gpu = pytest.mark.gpu

SUM, NORM = 1, 2
EPS = 1e-6
OUT = ("C", "den", "z")
GRADS = ("dxdst", "dxsrc", "dv", "de")
RTOL = 2e-4   # _close's


def compute(rp, ci, xd, xs, V, E, mode, eps, G=None, Gz=None, dt=np.float64):
    """Row by row in the arithmetic `dt`, from the fp32 inputs: {C, den, z} and, with G, {dxdst, dxsrc, dv, de}.  float64: the
    reference; float32: the emulation of the kernels (sequential sums)."""
    M, N = xd.shape
    K, nnz = xs.shape[0], len(ci)
    xd, xs, V = xd.astype(dt), xs.astype(dt), V.astype(dt)
    E = E.astype(dt) if E is not None else None
    one, eps = dt(1), dt(eps)
    res = {"C": np.zeros((M, N), dt), "den": np.zeros((M, N), dt), "z": np.zeros((nnz, N), dt)}
    if G is not None:
        G = G.astype(dt)
        Gz = Gz.astype(dt) if Gz is not None else None
        res.update(dxdst=np.zeros((M, N), dt), dxsrc=np.zeros((K, N), dt), dv=np.zeros((K, N), dt), de=np.zeros((nnz, N), dt))
    seq = lambda x: np.cumsum(x, axis=0, dtype=dt)[-1]   # noqa: E731  (in the order of the entries)
    for r in range(M):
        b, e = int(rp[r]), int(rp[r + 1])
        if e == b:
            continue
        c = ci[b:e]
        z = xd[r] + xs[c]
        if E is not None:
            z = z + E[b:e]
        with np.errstate(over="ignore"):
            g = one / (one + np.exp(-z))
        num, den = seq(g * V[c]), seq(g)
        C = num / (den + eps) if mode == NORM else num
        res["z"][b:e], res["den"][r], res["C"][r] = z, den, C
        if G is not None:
            gn = G[r] / (den + eps) if mode == NORM else G[r]
            dz = gn * (V[c] - (C if mode == NORM else dt(0))) * (g * (one - g))
            if Gz is not None:
                dz = dz + Gz[b:e]
            res["de"][b:e], res["dxdst"][r] = dz, seq(dz)
            np.add.at(res["dxsrc"], c, dz)
            np.add.at(res["dv"], c, g * gn)
    return res


def share(got, want):
    """the largest part of _close's limit that got uses"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err, limit = np.abs(got - want), RTOL * (np.abs(want) + np.abs(want).max() * 1e-2)
    with np.errstate(divide="ignore", invalid="ignore"):   # (an all-zero reference: the limit is 0)
        return float(np.where(limit > 0, err / limit, np.where(err > 0, np.inf, 0.0)).max())


_refs = {}


def base_case(N, mode, with_e):
    """the 400 x 300 matrix of the reduce tests (empty rows, one row of 300), the operands, G, Gz and the float64 reference, once per case"""
    key = (N, mode, with_e)
    if key not in _refs:
        rs, rp, ci, _, M, K = base_matrix(5)
        nnz = len(ci)
        xd, xs, V, G = rand(rs, M, N), rand(rs, K, N), rand(rs, K, N), rand(rs, M, N)
        E, Gz = rand(rs, nnz, N), rand(rs, nnz, N)
        E = E if with_e else None
        _refs[key] = (rp, ci, M, K, xd, xs, V, E, G, Gz, compute(rp, ci, xd, xs, V, E, mode, EPS, G, Gz))
    return _refs[key]


@pytest.mark.parametrize("with_e", [False, True])
@pytest.mark.parametrize("mode", [SUM, NORM])
def test_emulation_stays_under_half_the_limit(mode, with_e):
    rp, ci, M, K, xd, xs, V, E, G, Gz, want = base_case(16, mode, with_e)
    emu = compute(rp, ci, xd, xs, V, E, mode, EPS, G, Gz, dt=np.float32)
    shares = {k: share(emu[k], want[k]) for k in OUT + GRADS}
    print(mode, with_e, {k: round(s, 4) for k, s in shares.items()})
    assert max(shares.values()) < 0.5, shares
    assert all(emu[k].dtype == np.float32 for k in emu)


class GatedAbi(Abi):
    """test_spmm_reduce_gpu.Abi's engine on a pattern (values 1: never read), the gated aggregation's entry points through api.Engine"""

    def __init__(self, sx, rp, ci, M, K):
        super().__init__(sx, rp, ci, np.ones(len(ci), np.float32), M, K)
        self.sx = sx

    def operands(self, xd, xs, V, E, pad=0):
        """-> (GatedIn, the device tensors it points to); pad: extra columns of every operand buffer"""
        tc = self.t
        N = xd.shape[1]
        keep = []
        gin = self.sx.api.GatedIn()
        for name, x in (("xdst", xd), ("xsrc", xs), ("v", V), ("e", E)):
            if x is None:
                continue
            buf = tc.zeros((max(x.shape[0], 1), N + pad), device="cuda")
            buf[:x.shape[0], :N] = tc.from_numpy(np.ascontiguousarray(x))
            keep.append(buf)
            setattr(gin, "d_" + name, buf.data_ptr())
            setattr(gin, "ld_" + name, N + pad)
        return gin, keep

    def fwd(self, mode, xd, xs, V, E=None, want=OUT, pad=(0, 0), eps=EPS):
        """-> {C, den, z} as numpy float32 and {name + "_buf"}: the whole padded int32 buffers; the outputs not in `want` get no pointer
        and must keep their POISON; pad: extra columns of the operand / output buffers"""
        tc = self.t
        N = xd.shape[1]
        gin, keep = self.operands(xd, xs, V, E, pad[0])
        rows = {"C": self.M, "den": self.M, "z": max(self.nnz, 1)}
        buf = {k: tc.full((rows[k], N + pad[1]), POISON, dtype=tc.int32, device="cuda") for k in OUT}
        p = {k: (buf[k].data_ptr() if k in want else None) for k in OUT}
        ld = N + pad[1]
        self.eng.spmm_gated_device_rm(mode, eps, N, gin, p["C"], ld, p["den"], ld, p["z"], ld, tc.cuda.current_stream().cuda_stream)
        tc.cuda.synchronize()
        out = {}
        for k in OUT:
            full = buf[k].cpu().numpy()[:self.nnz if k == "z" else self.M]
            out[k], out[k + "_buf"] = full[:, :N].view(np.float32), full
        return out

    def bwd(self, mode, xd, xs, V, E, f, G, Gz=None, want=GRADS, pad=(0, 0), eps=EPS):
        """-> {name: numpy} of the four gradients (whole padded buffers under name + "_buf"): the ones not in `want` get no pointer and
        must keep their 7.0; f: the forward's outputs"""
        tc = self.t
        N = G.shape[1]
        gin, keep = self.operands(xd, xs, V, E, pad[0])
        Ct, Dt, Gt = (tc.from_numpy(np.ascontiguousarray(x)).cuda() for x in (f["C"], f["den"], G))
        Gzt = tc.from_numpy(np.ascontiguousarray(Gz)).cuda() if Gz is not None else None
        nwork = self.eng.spmm_gated_workspace_floats(mode, N)
        assert nwork == (self.M * N if mode == NORM else 0)
        work = tc.full((max(nwork, 4),), 7.0, device="cuda")
        rows = {"dxdst": self.M, "dxsrc": self.K, "dv": self.K, "de": max(self.nnz, 1)}
        buf = {k: tc.full((rows[k], N + pad[1]), 7.0, device="cuda") for k in GRADS}
        out = self.sx.api.GatedGrad()
        for k in GRADS:
            if k in want:
                setattr(out, "d_" + k, buf[k].data_ptr())
            setattr(out, "ld_" + k, N + pad[1])
        self.eng.spmm_gated_backward_device_rm(mode, eps, N, gin, Ct.data_ptr(), N, Dt.data_ptr(), N, Gt.data_ptr(), N,
                                               Gzt.data_ptr() if Gzt is not None else None, N, out, work.data_ptr() if nwork else None,
                                               tc.cuda.current_stream().cuda_stream)
        tc.cuda.synchronize()
        res = {}
        for k in GRADS:
            full = buf[k].cpu().numpy()[:self.nnz if k == "de" else rows[k]]
            res[k], res[k + "_buf"] = full[:, :N], full
        return res


def check(got, want, names, where):
    for k in names:
        print(where, k, "share of the limit %.4f" % share(got[k], want[k]))
        assert _close(got[k], want[k]), (where, k)
        assert np.all(np.isfinite(got[k])), (where, k)


@gpu
@pytest.mark.parametrize("with_e", [False, True])
@pytest.mark.parametrize("mode", [SUM, NORM])
@pytest.mark.parametrize("N", [8, 16, 24, 64, 72, 136])
def test_forward_and_backward_on_the_c_abi(sx, N, mode, with_e):
    """one tile, a partial last tile, several tiles; both modes, with and without E; the exact bits of z and of empty rows; padded
    leading dimensions; optional outputs; each gradient alone"""
    rp, ci, M, K, xd, xs, V, E, G, Gz, want = base_case(N, mode, with_e)
    a = GatedAbi(sx, rp, ci, M, K)
    f = a.fwd(mode, xd, xs, V, E)
    assert a.eng.last_kernel() == "spmm_gated"
    check(f, want, OUT, (N, mode, with_e))
    z32 = xd[np.repeat(np.arange(M), np.diff(rp))] + xs[ci]   # numpy float32: one rounded add, then E's
    z32 = z32 + E if with_e else z32
    assert z32.dtype == np.float32 and bits_equal(f["z"], z32)
    empty = np.flatnonzero(np.diff(rp) == 0)
    assert len(empty) > 10
    assert np.all(f["C"][empty].view(np.uint32) == 0) and np.all(f["den"][empty].view(np.uint32) == 0)
    # padded leading dimensions: the same bits, the padding left alone
    f2 = a.fwd(mode, xd, xs, V, E, pad=(4, 8))
    for k in OUT:
        assert same(f2[k], f[k]) and np.all(f2[k + "_buf"][:, N:] == POISON), k
    # outputs given no pointer stay untouched
    f2 = a.fwd(mode, xd, xs, V, E, want=("C",))
    assert same(f2["C"], f["C"]) and np.all(f2["den_buf"] == POISON) and np.all(f2["z_buf"] == POISON)
    f2 = a.fwd(mode, xd, xs, V, E, want=("C", "z"))
    assert same(f2["C"], f["C"]) and same(f2["z"], f["z"]) and np.all(f2["den_buf"] == POISON)

    got = a.bwd(mode, xd, xs, V, E, f, G, Gz)
    assert a.eng.last_kernel() == "spmm_gated_backward"
    check(got, want, GRADS, (N, mode, with_e))
    assert np.all(got["dxdst"][empty] == 0)
    g2 = a.bwd(mode, xd, xs, V, E, f, G, Gz, pad=(8, 4))
    for k in GRADS:
        assert same(g2[k], got[k]) and np.all(g2[k + "_buf"][:, N:] == 7.0), k
    # each gradient alone: the same bits, the others' buffers keep their fill
    for k in GRADS:
        alone = a.bwd(mode, xd, xs, V, E, f, G, Gz, want=(k,))
        assert same(alone[k], got[k]), k
        for other in GRADS:
            if other != k:
                assert np.all(alone[other + "_buf"] == 7.0), (k, other)
    # no Gz: the gradient through C alone
    w0 = compute(rp, ci, xd, xs, V, E, mode, EPS, G, None)
    check(a.bwd(mode, xd, xs, V, E, f, G, None), w0, GRADS, (N, mode, with_e, "no Gz"))
    a.eng.close()


@gpu
@pytest.mark.parametrize("with_e", [False, True])
@pytest.mark.parametrize("mode", [SUM, NORM])
def test_saturated_gates(sx, mode, with_e):
    """x_dst = +200: every gate is exactly 1 -- den is the row length, a single-entry row's C has V[c]'s bits in SUM mode; x_dst = -200:
    every gate is exactly +0 -- C and every gradient through the gate are +-0; no NaN or inf anywhere"""
    N = 24
    rp0, ci0, M, K, xd, xs, V, E0, G, Gz, _ = base_case(N, mode, True)
    rp, ci, keep = cut_rows(rp0, ci0, np.arange(len(ci0), dtype=np.float32))   # every eighth row cut down to its first entry
    E = E0[keep.astype(np.int64)] if with_e else None
    lens = np.diff(rp)
    single = np.flatnonzero(lens == 1)
    assert len(single) >= 40 and np.all(V != 0)
    a = GatedAbi(sx, rp, ci, M, K)
    hot = np.full_like(xd, 200.0)
    f = a.fwd(mode, hot, xs, V, E)
    assert np.array_equal(f["den"], np.repeat(lens[:, None], N, 1).astype(np.float32))
    if mode == SUM:
        assert bits_equal(f["C"][single], V[ci[rp[single]]])
    want = compute(rp, ci, hot, xs, V, E, mode, EPS, G, None)
    check(f, want, OUT, ("hot", mode, with_e))
    got = a.bwd(mode, hot, xs, V, E, f, G, None)
    check(got, want, GRADS, ("hot", mode, with_e))
    for k in ("dxdst", "dxsrc", "de"):
        assert np.all(got[k] == 0), k
    cold = np.full_like(xd, -200.0)
    f = a.fwd(mode, cold, xs, V, E)
    assert np.all(f["C"] == 0) and np.all(f["den"] == 0) and np.all(np.isfinite(f["z"]))
    got = a.bwd(mode, cold, xs, V, E, f, G, None)
    for k in GRADS:
        assert np.all(got[k] == 0), k
    # with Gz the gate's share is still +-0: dE is Gz itself, dxdst its row sums
    got = a.bwd(mode, cold, xs, V, E, f, G, Gz[keep.astype(np.int64)])
    assert bits_equal(got["de"], Gz[keep.astype(np.int64)]) and np.all(got["dv"] == 0)
    assert all(np.all(np.isfinite(got[k])) for k in GRADS)
    a.eng.close()


@gpu
@pytest.mark.parametrize("mode", [SUM, NORM])
def test_long_rows(sx, mode):
    """rows of 1 .. 300 entries, one of 2500 (the workgroup path) and a column of more than 2048 entries (the column pass's)"""
    rs = np.random.RandomState(8)
    rp, ci, _, M, K = edge_pattern(rs)
    assert M < 3000 and np.count_nonzero(ci == 0) > 2048 and np.diff(rp).max() == 2500
    N, nnz = 24, len(ci)
    xd, xs, V, G, E, Gz = rand(rs, M, N), rand(rs, K, N), rand(rs, K, N), rand(rs, M, N), rand(rs, nnz, N), rand(rs, nnz, N)
    want = compute(rp, ci, xd, xs, V, E, mode, EPS, G, Gz)
    a = GatedAbi(sx, rp, ci, M, K)
    f = a.fwd(mode, xd, xs, V, E)
    assert a.eng.last_kernel() == "spmm_gated+long_rows"
    got = a.bwd(mode, xd, xs, V, E, f, G, Gz)
    assert a.eng.last_kernel() == "spmm_gated_backward+long_rows"
    a.eng.close()
    check(f, want, OUT, ("long", mode))
    check(got, want, GRADS, ("long", mode))


@gpu
@pytest.mark.parametrize("name", ["P", "PT"])
@pytest.mark.parametrize("N", [8, 16, 32, 64])
def test_row_dealing(sx, N, name):
    """test_pattern_dealing_gpu's pattern (slot groups E = 1 .. S, the second walk, long rows, empty rows) and its transpose, at one
    width per slot shape; GatedGCN's full call: NORM, E, Gz"""
    p, rs = pat(name), rng("gated", N, name)
    xd, xs, V, G = rand(rs, p.M, N), rand(rs, p.K, N), rand(rs, p.K, N), rand(rs, p.M, N)
    E, Gz = rand(rs, p.nnz, N), rand(rs, p.nnz, N)
    a = GatedAbi(sx, p.rp, p.ci, p.M, p.K)
    f = a.fwd(NORM, xd, xs, V, E)
    fwd = a.eng.last_kernel()
    got = a.bwd(NORM, xd, xs, V, E, f, G, Gz)
    names_ok(p, "spmm_gated", fwd, a.eng.last_kernel())
    a.eng.close()
    want = compute(p.rp, p.ci, xd, xs, V, E, NORM, EPS, G, Gz)
    check(f, want, OUT, (name, N))
    check(got, want, GRADS, (name, N))
    assert np.all(f["C"][p.empty].view(np.uint32) == 0) and np.all(f["den"][p.empty].view(np.uint32) == 0)
    assert np.all(got["dxdst"][p.empty] == 0)


@gpu
@pytest.mark.parametrize("mode", [SUM, NORM])
def test_degenerate_matrices(sx, mode):
    """no entry at all: C, den, dxdst, dxsrc and dV are zero-filled (the padding left alone), z and dE have no element; no row at all"""
    import torch
    from sextans_amd import torch_op
    from sextans_amd.gated import spmm_gated
    rs = np.random.RandomState(3)
    M, K, N = 5, 6, 16
    xd, xs, V, G = rand(rs, M, N), rand(rs, K, N), rand(rs, K, N), rand(rs, M, N)
    none = np.zeros((0, N), np.float32)
    a = GatedAbi(sx, np.zeros(M + 1, np.int32), np.zeros(0, np.int32), M, K)
    f = a.fwd(mode, xd, xs, V, none, pad=(0, 4))
    for k in ("C", "den"):
        assert np.all(f[k].view(np.uint32) == 0) and np.all(f[k + "_buf"][:, N:] == POISON), k
    assert f["z"].shape[0] == 0
    g = a.bwd(mode, xd, xs, V, none, f, G, none, pad=(0, 4))
    for k in GRADS[:3]:
        assert np.all(g[k] == 0) and np.all(g[k + "_buf"][:, N:] == 7.0), k
    assert g["de"].shape[0] == 0
    a.eng.close()
    z = GatedAbi(sx, np.zeros(1, np.int32), np.zeros(0, np.int32), 0, K)
    f = z.fwd(mode, np.zeros((0, N), np.float32), xs, V, None)
    assert f["C"].shape[0] == 0
    g = z.bwd(mode, np.zeros((0, N), np.float32), xs, V, None, f, np.zeros((0, N), np.float32))
    assert g["dxdst"].shape[0] == 0 and np.all(g["dxsrc"] == 0) and np.all(g["dv"] == 0)
    z.eng.close()
    # the same through the torch op
    torch_op.clear_cache()
    A = make_A(np.zeros(M + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), M, K)
    ops = [torch.from_numpy(x).cuda().requires_grad_() for x in (xd, xs, V, none)]
    C, ze = spmm_gated(A, *ops, normalize=mode == NORM, return_edge=True)
    assert C.shape == (M, N) and ze.shape == (0, N) and not C.any()
    C.backward(torch.from_numpy(G).cuda())
    assert all(t.grad is not None and not t.grad.any() for t in ops[:3]) and ops[3].grad.shape == (0, N)
    torch_op.clear_cache()


@gpu
def test_determinism_streams_and_graph_replay(sx):
    import torch
    N, mode = 24, NORM
    rp, ci, M, K, xd, xs, V, E, G, Gz, _ = base_case(N, mode, True)
    G2 = rand(np.random.RandomState(77), M, N)
    a = GatedAbi(sx, rp, ci, M, K)

    def both(Gn):
        f = a.fwd(mode, xd, xs, V, E)
        g = a.bwd(mode, xd, xs, V, E, f, Gn, Gz)
        return [f[k] for k in OUT] + [g[k] for k in GRADS]

    first, second = both(G), both(G)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = both(G)
    torch.cuda.current_stream().wait_stream(side)
    for i, (x, y, z) in enumerate(zip(first, second, third)):
        assert same(x, y) and same(x, z), i
    want = both(G2)
    assert not same(want[3], first[3])

    # the backward captured on a side stream (tables exist: the calls above were the warm-up), replayed with another G
    tc = torch
    gin, keep = a.operands(xd, xs, V, E)
    Ct, Dt, Gt, Gzt = (tc.from_numpy(np.ascontiguousarray(x)).cuda() for x in (first[0], first[1], G, Gz))
    bufs = [tc.zeros((M, N), device="cuda"), tc.zeros((K, N), device="cuda"), tc.zeros((K, N), device="cuda"), tc.zeros((a.nnz, N), device="cuda")]
    out = sx.api.GatedGrad()
    for k, b in zip(GRADS, bufs):
        setattr(out, "d_" + k, b.data_ptr())
        setattr(out, "ld_" + k, N)
    work = tc.zeros((a.eng.spmm_gated_workspace_floats(mode, N),), device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        a.eng.spmm_gated_backward_device_rm(mode, EPS, N, gin, Ct.data_ptr(), N, Dt.data_ptr(), N, Gt.data_ptr(), N, Gzt.data_ptr(), N, out,
                                            work.data_ptr(), torch.cuda.current_stream().cuda_stream)
    Gt.copy_(tc.from_numpy(G2).cuda())
    g.replay()
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(bufs, want[3:])):
        assert same(x.cpu().numpy(), y), i
    a.eng.close()


def dense_torch_reference(rp, ci, M, K, xd, xs, V, E, normalize, eps, G, Gz):
    """a float64 composition on the CPU with torch's autograd through both outputs: (C, z, dxdst, dxsrc, dV, dE)"""
    import torch
    rows = torch.from_numpy(np.repeat(np.arange(M), np.diff(rp)))
    cols = torch.from_numpy(ci.astype(np.int64))
    ops = [torch.from_numpy(x.astype(np.float64)).requires_grad_() for x in (xd, xs, V, E)]
    xdt, xst, Vt, Et = ops
    z = xdt[rows] + xst[cols] + Et
    g = torch.sigmoid(z)
    C = torch.zeros((M, xd.shape[1]), dtype=torch.float64).index_add(0, rows, g * Vt[cols])
    if normalize:
        C = C / (torch.zeros((M, xd.shape[1]), dtype=torch.float64).index_add(0, rows, g) + eps)
    ((C * torch.from_numpy(G.astype(np.float64))).sum() + (z * torch.from_numpy(Gz.astype(np.float64))).sum()).backward()
    return [C.detach().numpy(), z.detach().numpy()] + [t.grad.numpy() for t in ops]


@gpu
@pytest.mark.parametrize("normalize", [False, True])
def test_torch_autograd_padding_and_errors(sx, normalize):
    """N = 20 (no multiple of 8) through the padded copies; gradients of all four operands through both outputs against the dense
    composition; return_edge=False; no E; one engine, no value refresh; errors"""
    import torch
    from sextans_amd import torch_op
    from sextans_amd.gated import spmm_gated
    N = 20
    rs, rp, ci, v, M, K = base_matrix(5)
    nnz = len(ci)
    xd, xs, V, E = rand(rs, M, N), rand(rs, K, N), rand(rs, K, N), rand(rs, nnz, N)
    G, Gz = rand(rs, M, N), rand(rs, nnz, N)
    want = dense_torch_reference(rp, ci, M, K, xd, xs, V, E, normalize, 1e-6, G, Gz)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    ops = [torch.from_numpy(x).cuda().requires_grad_() for x in (xd, xs, V, E)]
    C, z = spmm_gated(A, *ops, normalize=normalize, return_edge=True)
    assert C.shape == (M, N) and z.shape == (nnz, N) and C.requires_grad and z.requires_grad
    ((C * torch.from_numpy(G).cuda()).sum() + (z * torch.from_numpy(Gz).cuda()).sum()).backward()
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0, info
    got = [C, z] + [t.grad for t in ops]
    for name, g, w in zip(("C", "z", "dxdst", "dxsrc", "dV", "dE"), got, want):
        g = g.detach().cpu().numpy()
        assert g.shape == w.shape, name
        print(name, "share of the limit %.4f" % share(g, w))
        assert _close(g, w), name
    # return_edge=False and no autograd: the same C bits
    det = [t.detach() for t in ops]
    assert same(spmm_gated(A, *det, normalize=normalize).cpu().numpy(), C.detach().cpu().numpy())
    C2 = spmm_gated(A, *ops, normalize=normalize)
    assert same(C2.detach().cpu().numpy(), C.detach().cpu().numpy())
    # only z used downstream; only C used, E without a gradient
    for t in ops:
        t.grad = None
    _, z2 = spmm_gated(A, *ops, normalize=normalize, return_edge=True)
    (z2 * torch.from_numpy(Gz).cuda()).sum().backward()
    assert _close(ops[3].grad.cpu().numpy(), Gz) and np.all(ops[2].grad.cpu().numpy() == 0)
    # no E
    w3 = compute(rp, ci, xd, xs, V, None, NORM if normalize else SUM, 1e-6, G, None)
    for t in ops:
        t.grad = None
    C3 = spmm_gated(A, ops[0], ops[1], ops[2], normalize=normalize, fast=True)
    C3.backward(torch.from_numpy(G).cuda())
    assert _close(C3.detach().cpu().numpy(), w3["C"])
    for k, t in zip(GRADS[:3], ops[:3]):
        assert _close(t.grad.cpu().numpy(), w3[k]), k
    assert torch_op.cache_info()["value_refreshes"] == 0
    with pytest.raises(TypeError):
        spmm_gated(A, det[0].cpu(), det[1], det[2])
    with pytest.raises(TypeError):
        spmm_gated(A.to_dense(), det[0], det[1], det[2])
    with pytest.raises(ValueError):
        spmm_gated(A, det[0][:-1], det[1], det[2])
    with pytest.raises(ValueError):
        spmm_gated(A, det[0], det[1], det[2][:, :-1])
    with pytest.raises(ValueError):
        spmm_gated(A, det[0], det[1], det[2], det[3][:-1])
    for bad in (0.0, -1e-6, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            spmm_gated(A, det[0], det[1], det[2], normalize=True, eps=bad)
    assert spmm_gated(A, det[0], det[1], det[2], normalize=False, eps=0.0).shape == (M, N)   # SUM ignores eps
    torch_op.clear_cache()
