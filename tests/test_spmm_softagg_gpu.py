"""Softmax aggregation SpMM on the GPU (sextans_spmm_softagg_device_rm / _backward_device_rm, torch_op.spmm_softagg): C, lse, dB, dval
and dt against a float64 numpy reference built row by row from the fp32-rounded products; exact bits where the arithmetic fixes them
(empty rows, rows of one entry, t = 1 against d_t = NULL); overflow safety at |t| = 200; every row-dealing path; determinism across
runs, streams and graph replay; the torch op with autograd in A, B and t.

Tolerance: test_torch_autograd_gpu._close (rtol 2e-4), the project's tolerance for fp32 sums.  A CPU emulation of the kernels' fp32
arithmetic stays under 0.11 of that limit for C, lse and the three gradients at the temperatures TEMPS; gradients are not compared
at |t| >= 100, where the factor t (p - C) amplifies the rounding of the score (the emulation of dB reaches 0.87 - 1.47 of the limit)."""
import numpy as np
import pytest

from test_fused_attention_gpu import edge_pattern, rand, same
from test_spmm_reduce_gpu import POISON, Abi, base_matrix, bits_equal
from test_torch_attention_gpu import make_A
from test_torch_autograd_gpu import _close

pytestmark = pytest.mark.gpu

TEMPS = [0, -3, 8, 1, 0.5, -8, 7, 2]
HOT = [200, -200, 100, -100]


def temps(N, cycle=TEMPS):
    return np.array([cycle[i % len(cycle)] for i in range(N)], np.float32)


def reference(rp, ci, v, B, t, G=None, K=None):
    """float64, row by row, from the fp32-rounded products: (C, lse) or, with G, (C, lse, dB, dval, dt).  t None = 1."""
    M, N = len(rp) - 1, B.shape[1]
    t64 = np.ones(N) if t is None else t.astype(np.float64)
    C, lse = np.zeros((M, N)), np.full((M, N), -np.inf)
    dB, dv, dt = (np.zeros((K, N)), np.zeros(len(ci)), np.zeros(N)) if G is not None else (None, None, None)
    for r in range(M):
        b, e = rp[r], rp[r + 1]
        if e == b:
            continue
        Br = B[ci[b:e]]
        P = (v[b:e, None] * Br).astype(np.float32).astype(np.float64)   # ONE rounded fp32 product
        s = t64 * P
        m = s.max(0)
        w = np.exp(s - m)
        z = w.sum(0)
        w /= z
        C[r] = (w * P).sum(0)
        lse[r] = m + np.log(z)
        if G is not None:
            d = P - C[r]
            q = G[r].astype(np.float64) * w * (1 + t64 * d)
            np.add.at(dB, ci[b:e], v[b:e, None].astype(np.float64) * q)
            dv[b:e] = (Br.astype(np.float64) * q).sum(1)
            dt += G[r].astype(np.float64) * (w * P * d).sum(0)
    return (C, lse) if G is None else (C, lse, dB, dv, dt)


def cut_rows(rp, ci, v, every=8):
    """the matrix with every `every`-th row cut down to its first entry (empty rows stay empty)"""
    lens = np.diff(rp)
    keep = np.ones(len(ci), bool)
    for r in range(0, len(lens), every):
        keep[rp[r] + 1:rp[r + 1]] = False
    lens1 = np.array([keep[rp[r]:rp[r + 1]].sum() for r in range(len(lens))])
    rp1 = np.zeros(len(rp), np.int32); rp1[1:] = np.cumsum(lens1)
    return rp1, ci[keep].copy(), v[keep].copy()


def lse_close(got, want):
    fin = np.isfinite(want)
    return np.array_equal(fin, np.isfinite(got)) and np.all(got[~fin] == -np.inf) and _close(got[fin], want[fin])


class SoftAbi(Abi):
    """test_spmm_reduce_gpu.Abi's engine on a matrix, the softmax aggregation's entry points called through api.Engine"""

    def fwd(self, B, t=None, val=None, want_lse=True, pad=(0, 0, 0), engine_values=False):
        """-> (C, lse) as numpy and the whole padded buffers as int32; pad: extra columns of the B / C / lse buffers"""
        tc = self.t
        N = B.shape[1]
        Bb = tc.zeros((self.K, N + pad[0]), device="cuda")
        Bb[:, :N] = tc.from_numpy(B)
        Cb = tc.full((self.M, N + pad[1]), POISON, dtype=tc.int32, device="cuda")
        Lb = tc.full((self.M, N + pad[2]), POISON, dtype=tc.int32, device="cuda")
        tt = tc.from_numpy(t).cuda() if t is not None else None
        vv = None if engine_values else (self.val if val is None else tc.from_numpy(val).cuda())
        self.eng.spmm_softagg_device_rm(N, vv.data_ptr() if vv is not None else None, Bb.data_ptr(), N + pad[0],
                                        tt.data_ptr() if tt is not None else None, Cb.data_ptr(), N + pad[1],
                                        Lb.data_ptr() if want_lse else None, N + pad[2], tc.cuda.current_stream().cuda_stream)
        tc.cuda.synchronize()
        Cn, Ln = Cb.cpu().numpy(), Lb.cpu().numpy()
        return Cn[:, :N].view(np.float32), Ln[:, :N].view(np.float32), Cn, Ln

    def bwd(self, B, t, C, lse, G, want=("dB", "dval", "dt"), work=True):
        """-> {name: numpy} of the three gradients and the workspace: the ones not in `want` get no pointer and must keep their 7.0"""
        tc = self.t
        N = G.shape[1]
        Bt, Ct, Lt, Gt = (tc.from_numpy(np.ascontiguousarray(x)).cuda() for x in (B, C, lse, G))
        tt = tc.from_numpy(t).cuda() if t is not None else None
        nwork = self.eng.spmm_softagg_workspace_floats(N)
        assert nwork == self.M * N + (self.M + 255) // 256 * N
        buf = {"dB": tc.full((self.K, N), 7.0, device="cuda"), "dval": tc.full((max(self.nnz, 4),), 7.0, device="cuda"),
               "dt": tc.full((N,), 7.0, device="cuda"), "work": tc.full((nwork,), 7.0, device="cuda")}
        p = {k: (x.data_ptr() if k in want or (k == "work" and work) else None) for k, x in buf.items()}
        self.eng.spmm_softagg_backward_device_rm(N, self.val.data_ptr(), Bt.data_ptr(), N, tt.data_ptr() if tt is not None else None,
                                                 Ct.data_ptr(), N, Lt.data_ptr(), N, Gt.data_ptr(), N, p["dB"], N, p["dval"], p["dt"],
                                                 p["work"], tc.cuda.current_stream().cuda_stream)
        tc.cuda.synchronize()
        out = {k: x.cpu().numpy() for k, x in buf.items()}
        out["dval"] = out["dval"][:self.nnz]
        return out


_refs = {}


def base_case(N, cycle="temps"):
    """the 400 x 300 matrix of the reduce tests (empty rows, one row of 300), B, G, t and the float64 reference, computed once per case"""
    key = (N, cycle)
    if key not in _refs:
        rs, rp, ci, v, M, K = base_matrix(5)
        B, G = rand(rs, K, N), rand(rs, M, N)
        t = {"temps": temps(N), "hot": temps(N, HOT), "none": None}[cycle]
        _refs[key] = (rp, ci, v, M, K, B, G, t, reference(rp, ci, v, B, t, G, K))
    return _refs[key]


@pytest.mark.parametrize("cycle", ["none", "temps"])
@pytest.mark.parametrize("N", [8, 16, 24, 64, 136, 264])
def test_forward_on_the_c_abi(sx, N, cycle):
    """one tile, several tiles and a partial last tile; d_t NULL and per-column temperatures; padded leading dimensions with the padding
    left alone; no lse; the engine's values; the exact bits of empty rows and of rows of one entry"""
    rp, ci, v, M, K, B, G, t, (wC, wL, _, _, _) = base_case(N, cycle)
    a = SoftAbi(sx, rp, ci, v, M, K)
    C, lse, _, _ = a.fwd(B, t)
    assert a.eng.last_kernel() == "spmm_softagg"
    print(N, cycle, "max |C - ref|", float(np.abs(C - wC).max()))
    assert _close(C, wC) and lse_close(lse, wL)
    empty = np.flatnonzero(np.diff(rp) == 0)
    assert len(empty) > 10
    assert np.all(C[empty].view(np.uint32) == 0) and np.all(lse[empty] == -np.inf)
    C2, lse2, Cb, Lb = a.fwd(B, t, pad=(4, 8, 12))
    assert same(C2, C) and same(lse2, lse)
    assert np.all(Cb[:, N:] == POISON) and np.all(Lb[:, N:] == POISON)
    C2, _, _, Lb = a.fwd(B, t, want_lse=False)
    assert same(C2, C) and np.all(Lb == POISON)
    C2, lse2, _, _ = a.fwd(B, t, engine_values=True)
    assert same(C2, C) and same(lse2, lse)
    a.eng.close()
    # rows of one entry (the matrix above has none: every eighth row cut down to its first entry): w = 1, z = 1, C has the product's bits
    rp1, ci1, v1 = cut_rows(rp, ci, v)
    single = np.flatnonzero(np.diff(rp1) == 1)
    assert len(single) >= 40
    a = SoftAbi(sx, rp1, ci1, v1, M, K)
    C, lse, _, _ = a.fwd(B, t)
    a.eng.close()
    w1 = reference(rp1, ci1, v1, B, t)
    assert _close(C, w1[0]) and lse_close(lse, w1[1])
    prod = (v1[rp1[single], None] * B[ci1[rp1[single]]]).astype(np.float32)
    assert np.all(prod != 0) and bits_equal(C[single], prod)


def test_overflow_safety_forward(sx):
    """t p far beyond +-88: only differences to the running maximum are exponentiated"""
    N = 16
    rp, ci, v, M, K, B, G, t, (wC, wL, _, _, _) = base_case(N, "hot")
    assert np.abs(t[None, :] * B).max() > 150
    a = SoftAbi(sx, rp, ci, v, M, K)
    C, lse, _, _ = a.fwd(B, t)
    full = np.diff(rp) > 0
    assert np.all(np.isfinite(C)) and np.all(np.isfinite(lse[full]))
    print("max |C - ref|", float(np.abs(C - wC).max()), "max |lse - ref|", float(np.abs(lse[full] - wL[full]).max()))
    assert _close(C, wC) and lse_close(lse, wL)
    a.eng.close()


@pytest.mark.parametrize("N", [8, 24, 136])
def test_backward_on_the_c_abi(sx, N):
    rp, ci, v, M, K, B, G, t, (wC, wL, wdB, wdv, wdt) = base_case(N)
    a = SoftAbi(sx, rp, ci, v, M, K)
    C, lse, _, _ = a.fwd(B, t)
    got = a.bwd(B, t, C, lse, G)
    assert a.eng.last_kernel() == "spmm_softagg_backward"
    for name, want in (("dB", wdB), ("dval", wdv), ("dt", wdt)):
        print(N, name, "max |got - ref|", float(np.abs(got[name] - want).max()), "of max |ref|", float(np.abs(want).max()))
        assert _close(got[name], want), name
    # the workspace holds the rows' shares of dt, then the chunk sums
    rows = got["work"][:M * N].reshape(M, N).astype(np.float64)
    assert _close(rows.sum(0), wdt) and np.all(rows[np.diff(rp) == 0] == 0)
    # each gradient alone: the same bits, the others' buffers untouched; without dt the workspace is not written either
    for name in ("dB", "dval", "dt"):
        alone = a.bwd(B, t, C, lse, G, want=(name,), work=True)
        assert same(alone[name], got[name]), name
        for other in ("dB", "dval", "dt"):
            if other != name:
                assert np.all(alone[other] == 7.0), (name, other)
        assert same(alone["work"], got["work"]) if name == "dt" else np.all(alone["work"] == 7.0), name
    alone = a.bwd(B, t, C, lse, G, want=("dB", "dval"), work=False)
    assert same(alone["dB"], got["dB"]) and same(alone["dval"], got["dval"]) and np.all(alone["dt"] == 7.0)
    # d_t NULL is t = 1
    ones = a.bwd(B, np.ones(N, np.float32), *a.fwd(B, np.ones(N, np.float32))[:2], G)
    null = a.bwd(B, None, *a.fwd(B, None)[:2], G)
    for name in ("dB", "dval", "dt"):
        assert _close(null[name], ones[name]), name
    a.eng.close()


def torch_run(rp, ci, v, M, K, B, t, G, grad_t=True):
    """forward + backward through torch_op: [C, lse, dB, dval, dt] as numpy"""
    import torch
    from sextans_amd import torch_op
    A = make_A(rp, ci, v, M, K, grad=True)
    Bt = torch.from_numpy(B).cuda().requires_grad_()
    tt = torch.from_numpy(t).cuda().requires_grad_(grad_t)
    out, lse = torch_op.spmm_softagg(A, Bt, tt, return_lse=True)
    out.backward(torch.from_numpy(G).cuda())
    res = [out, lse, Bt.grad, A.grad.values()] + ([tt.grad] if grad_t else [])
    return [x.detach().cpu().numpy() for x in res]


def test_row_length_edges_and_long_rows(sx):
    """rows of 1 .. 300 entries, one of 2500 (the workgroup path) and a column of more than 2048 entries (the column pass's)"""
    from sextans_amd import torch_op
    rs = np.random.RandomState(8)
    rp, ci, v, M, K = edge_pattern(rs)
    assert M < 3000 and np.count_nonzero(ci == 0) > 2048 and np.diff(rp).max() == 2500
    N = 24
    B, G, t = rand(rs, K, N), rand(rs, M, N), temps(N)
    want = reference(rp, ci, v, B, t, G, K)
    torch_op.clear_cache()
    import torch
    A = make_A(rp, ci, v, M, K, grad=True)
    Bt = torch.from_numpy(B).cuda().requires_grad_()
    tt = torch.from_numpy(t).cuda().requires_grad_()
    out, lse = torch_op.spmm_softagg(A, Bt, tt, return_lse=True)
    eng = next(iter(torch_op._cache.values())).eng
    assert eng.last_kernel() == "spmm_softagg+long_rows"
    out.backward(torch.from_numpy(G).cuda())
    assert eng.last_kernel() == "spmm_softagg_backward+long_rows"
    got = [x.detach().cpu().numpy() for x in (out, lse, Bt.grad, A.grad.values(), tt.grad)]
    for name, g, w in zip(("C", "lse", "dB", "dval", "dt"), got, want):
        print(name, "max |got - ref|", float(np.abs(g - w).max()), "of max |ref|", float(np.abs(w).max()))
        assert _close(g, w), name
    single = np.flatnonzero(np.diff(rp) == 1)   # (2101 rows, most of them on column 0)
    assert bits_equal(got[0][single], (v[rp[single], None] * B[ci[rp[single]]]).astype(np.float32))
    torch_op.clear_cache()


def test_limits(sx):
    """t = 0 is the mean of the row's products; torch_op with t = 1.0 is the ABI call with d_t NULL, bit for bit"""
    import torch
    from sextans_amd import torch_op
    N = 16
    rp, ci, v, M, K, B, G, t, _ = base_case(N)
    assert t[0] == 0 and t[8] == 0
    a = SoftAbi(sx, rp, ci, v, M, K)
    C, lse, _, _ = a.fwd(B, t)
    lens = np.diff(rp)
    mean = np.zeros((M, N))
    for r in range(M):
        if lens[r]:
            mean[r] = (v[rp[r]:rp[r + 1], None] * B[ci[rp[r]:rp[r + 1]]]).astype(np.float32).astype(np.float64).mean(0)
    assert _close(C[:, [0, 8]], mean[:, [0, 8]])
    full = lens > 0
    assert _close(lse[full][:, [0, 8]], np.log(lens[full])[:, None].repeat(2, 1))
    C1, lse1, _, _ = a.fwd(B, None)
    a.eng.close()
    torch_op.clear_cache()
    A0, B0 = make_A(rp, ci, v, M, K), torch.from_numpy(B).cuda()
    Ct, lset = torch_op.spmm_softagg(A0, B0, t=1.0, return_lse=True)
    assert same(Ct.cpu().numpy(), C1) and same(lset.cpu().numpy(), lse1)
    assert same(torch_op.spmm_softagg(A0, B0).cpu().numpy(), C1)
    assert same(torch_op.spmm_softagg(A0, B0, fast=True).cpu().numpy(), C1)
    torch_op.clear_cache()


def test_determinism_streams_and_graph_replay(sx):
    import torch
    N = 24
    rp, ci, v, M, K, B, G, t, _ = base_case(N)
    rs = np.random.RandomState(77)
    G2 = rand(rs, M, N)
    a = SoftAbi(sx, rp, ci, v, M, K)

    def both(Gn):
        C, lse, _, _ = a.fwd(B, t)
        g = a.bwd(B, t, C, lse, Gn)
        return [C, lse, g["dB"], g["dval"], g["dt"]]

    first, second = both(G), both(G)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = both(G)
    torch.cuda.current_stream().wait_stream(side)
    for i, (x, y, z) in enumerate(zip(first, second, third)):
        assert same(x, y) and same(x, z), i
    want = both(G2)
    assert not same(want[2], first[2])

    # the backward captured on a side stream (tables exist: the calls above were the warm-up), replayed with another G
    tc = torch
    Bt, Ct, Lt, tt = (tc.from_numpy(np.ascontiguousarray(x)).cuda() for x in (B, first[0], first[1], t))
    Gt = tc.from_numpy(G).cuda()
    dB, dv, dt = tc.zeros((K, N), device="cuda"), tc.zeros((a.nnz,), device="cuda"), tc.zeros((N,), device="cuda")
    work = tc.zeros((a.eng.spmm_softagg_workspace_floats(N),), device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        a.eng.spmm_softagg_backward_device_rm(N, a.val.data_ptr(), Bt.data_ptr(), N, tt.data_ptr(), Ct.data_ptr(), N, Lt.data_ptr(), N,
                                              Gt.data_ptr(), N, dB.data_ptr(), N, dv.data_ptr(), dt.data_ptr(), work.data_ptr(),
                                              torch.cuda.current_stream().cuda_stream)
    Gt.copy_(tc.from_numpy(G2).cuda())
    g.replay()
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip((dB, dv, dt), want[2:])):
        assert same(x.cpu().numpy(), y), i
    a.eng.close()


def dense_torch_reference(rp, ci, v, M, K, B, t, G):
    """a dense float64 composition on the CPU with torch's autograd: (C, dB, dval, dt)"""
    import torch
    rows = torch.from_numpy(np.repeat(np.arange(M), np.diff(rp)))
    cols = torch.from_numpy(ci.astype(np.int64))
    vt = torch.from_numpy(v.astype(np.float64)).requires_grad_()
    Bt = torch.from_numpy(B.astype(np.float64)).requires_grad_()
    tt = torch.from_numpy(t.astype(np.float64)).requires_grad_()
    Ad = torch.zeros((M, K), dtype=torch.float64).index_put((rows, cols), vt)
    mask = torch.zeros((M, K), dtype=torch.bool)
    mask[rows, cols] = True
    P = Ad[:, :, None] * Bt[None, :, :]
    s = torch.where(mask[:, :, None], tt * P, torch.tensor(-np.inf, dtype=torch.float64))
    s = torch.where(mask.any(1)[:, None, None], s, torch.zeros((), dtype=torch.float64))   # (an empty row: no NaN in the softmax)
    w = torch.softmax(s, 1) * mask[:, :, None]
    C = (w * P).sum(1)
    C.backward(torch.from_numpy(G.astype(np.float64)))
    return C.detach().numpy(), Bt.grad.numpy(), vt.grad.numpy(), tt.grad.numpy()


def test_torch_autograd_padding_and_errors(sx):
    """N = 20 (no multiple of 8) through the padded copies; gradients of A, B and an (N,) t against the dense composition; a scalar t;
    lse; errors; no value refresh"""
    import torch
    from sextans_amd import torch_op
    N = 20
    rs, rp, ci, v, M, K = base_matrix(5)
    B, G, t = rand(rs, K, N), rand(rs, M, N), temps(N)
    wC, wdB, wdv, wdt = dense_torch_reference(rp, ci, v, M, K, B, t, G)
    torch_op.clear_cache()
    C, lse, dB, dv, dt = torch_run(rp, ci, v, M, K, B, t, G)
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0, info
    assert C.shape == (M, N) and lse.shape == (M, N) and dB.shape == (K, N) and dt.shape == (N,)
    for name, g, w in (("C", C, wC), ("dB", dB, wdB), ("dval", dv, wdv), ("dt", dt, wdt)):
        print(name, "max |got - ref|", float(np.abs(g - w).max()), "of max |ref|", float(np.abs(w).max()))
        assert _close(g, w), name
    # a t that needs no gradient: the same bits for the others, no workspace
    C2, lse2, dB2, dv2 = torch_run(rp, ci, v, M, K, B, t, G, grad_t=False)
    assert same(C2, C) and same(lse2, lse) and same(dB2, dB) and same(dv2, dv)
    # a scalar temperature: a 0-d gradient, the sum of the vector one
    A = make_A(rp, ci, v, M, K, grad=True)
    Bt = torch.from_numpy(B).cuda().requires_grad_()
    Gt = torch.from_numpy(G).cuda()
    t0 = torch.tensor(0.75, device="cuda", requires_grad=True)
    out, lse0 = torch_op.spmm_softagg(A, Bt, t0, return_lse=True)
    assert out.requires_grad and not lse0.requires_grad and lse0.shape == (M, N)
    out.backward(Gt)
    tv = torch.full((N,), 0.75, device="cuda", requires_grad=True)
    outv = torch_op.spmm_softagg(A, Bt, tv)
    outv.backward(Gt)
    assert same(out.detach().cpu().numpy(), outv.detach().cpu().numpy())
    assert t0.grad.shape == () and _close(t0.grad.cpu().numpy(), tv.grad.sum().cpu().numpy())
    # a Python float is that temperature everywhere
    assert same(torch_op.spmm_softagg(A.detach(), Bt.detach(), 0.75).cpu().numpy(), out.detach().cpu().numpy())
    with pytest.raises(TypeError):
        torch_op.spmm_softagg(A.detach(), Bt.detach().cpu())
    with pytest.raises(ValueError):
        torch_op.spmm_softagg(A.detach(), Bt.detach(), torch.ones(N + 1, device="cuda"))
    with pytest.raises(ValueError):
        torch_op.spmm_softagg(A.detach(), Bt.detach(), torch.ones((1, N), device="cuda"))
    assert torch_op.cache_info()["value_refreshes"] == 0
    torch_op.clear_cache()
