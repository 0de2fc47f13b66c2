"""sparse_attention(fused=True) and the C ABI under it (sextans_attention_device, sextans_attention_backward_device): one kernel pass per
direction for all heads, against the float64 dense masked attention per head (forward and every gradient) with the tolerance the
composition is held to (test_torch_autograd_gpu._close, rtol 2e-4); row lengths around every lane-group size and beyond the long-row
threshold; empty rows, unused columns and -inf masks; agreement with the composition; bit-reproducibility and a captured training step;
operands read where they lie.  Every row takes part in every comparison, except where a row is made NaN on purpose: there the test
asserts that at least 99 % of the rows (columns) are compared."""
import numpy as np
import pytest

from test_torch_attention_gpu import dense_attention, make_A, pattern
from test_torch_autograd_gpu import _close

pytestmark = pytest.mark.gpu

LR = 0.05
INVALID = 9


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def rand(rs, *shape):
    return rs.uniform(-1, 1, shape).astype(np.float32)


def reference(rp, ci, v, M, K, Qn, Kn, Vn, Gn, scale, bias):
    """float64 dense masked attention head by head: O (M, H, dv), dQ, dK, dV and the bias gradient summed over the heads"""
    import torch
    H = Qn.shape[1]
    out = {k: [] for k in ("O", "dQ", "dK", "dV")}
    dA = 0.0
    for h in range(H):
        want, _, (Qd, Kd, Vd, Avd), _ = dense_attention(rp, ci, v, M, K, np.ascontiguousarray(Qn[:, h]), np.ascontiguousarray(Kn[:, h]),
                                                        np.ascontiguousarray(Vn[:, h]), scale, bias)
        want.backward(torch.from_numpy(np.ascontiguousarray(Gn[:, h])).cuda().double())
        out["O"].append(want.detach().cpu().numpy())
        out["dQ"].append(Qd.grad.cpu().numpy()); out["dK"].append(Kd.grad.cpu().numpy()); out["dV"].append(Vd.grad.cpu().numpy())
        if bias:
            dA = dA + Avd.grad.cpu().numpy()
    res = {k: np.stack(x, axis=1) for k, x in out.items()}
    res["dA"] = dA
    return res


def run(rp, ci, v, M, K, Qn, Kn, Vn, Gn, scale, bias, fused, squeeze=False):
    """-> (O, dQ, dK, dV, dA values or None) as numpy, heads on axis 1; squeeze: hand H = 1 operands over as 2-D tensors"""
    import torch
    from sextans_amd import torch_op
    A = make_A(rp, ci, v, M, K, grad=bias)
    Q, Kt, V = (torch.from_numpy(t[:, 0] if squeeze else t).cuda().requires_grad_() for t in (Qn, Kn, Vn))
    out = torch_op.sparse_attention(A, Q, Kt, V, scale=scale, bias=bias, fused=fused)
    assert out.dim() == V.dim()
    out.backward(torch.from_numpy(Gn[:, 0] if squeeze else Gn).cuda())
    if bias:
        assert A.grad.layout == torch.sparse_csr and A.grad.values().dtype == A.values().dtype
    else:
        assert A.grad is None
    res = [t.detach().cpu().numpy() for t in (out, Q.grad, Kt.grad, V.grad)]
    if squeeze:
        res = [t[:, None] for t in res]
    return res + [A.grad.values().cpu().numpy() if bias else None]


def check(got, want, bias):
    for g, k in zip(got, ("O", "dQ", "dK", "dV")):
        assert g.shape == want[k].shape, k
        assert np.all(np.isfinite(g)), k
        assert _close(g, want[k]), (k, float(np.abs(g - want[k]).max()))
    if bias:
        assert _close(got[4], want["dA"]), ("dA", float(np.abs(got[4] - want["dA"]).max()))


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("H, d, dv", [(1, 16, 16), (3, 8, 24), (2, 64, 64), (2, 20, 40), (1, 128, 128)])
def test_against_dense_float64(sx, H, d, dv, bias):
    from sextans_amd import torch_op
    M, K = 300, 260
    rs, rp, ci, v = pattern(31 + d, M, K, 9)
    assert np.all(np.diff(rp) > 0)
    Qn, Kn, Vn, Gn = rand(rs, M, H, d), rand(rs, K, H, d), rand(rs, K, H, dv), rand(rs, M, H, dv)
    scale = None if d == 16 else 0.37
    torch_op.clear_cache()
    got = run(rp, ci, v, M, K, Qn, Kn, Vn, Gn, scale, bias, True, squeeze=(H == 1 and d == 16))
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0, info
    want = reference(rp, ci, v, M, K, Qn, Kn, Vn, Gn, 1.0 / np.sqrt(d) if scale is None else scale, bias)
    check(got, want, bias)
    torch_op.clear_cache()


def edge_pattern(rs):
    """rows of 1 .. 300 entries around every lane-group size, one row of 2500 (beyond the long-row threshold of 2048), and 2100 rows that
    hold column 0 alone, so that column 0 is a long row of A^T"""
    K = 2600
    lens = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 300, 2500] + [1] * 2100
    M = len(lens)
    rp = np.zeros(M + 1, np.int32); rp[1:] = np.cumsum(lens)
    ci = np.zeros(rp[-1], np.int32)
    for r in range(12):
        ci[rp[r]:rp[r + 1]] = np.sort(rs.choice(K, size=lens[r], replace=False))
    return rp, ci, rand(rs, rp[-1]), M, K


def test_row_length_edges_and_long_rows(sx):
    from sextans_amd import torch_op
    rs = np.random.RandomState(8)
    rp, ci, v, M, K = edge_pattern(rs)
    assert M < 3000 and np.count_nonzero(ci == 0) > 2048 and np.diff(rp).max() == 2500
    H, d = 2, 16
    Qn, Kn, Vn, Gn = rand(rs, M, H, d), rand(rs, K, H, d), rand(rs, K, H, d), rand(rs, M, H, d)
    torch_op.clear_cache()
    got = run(rp, ci, v, M, K, Qn, Kn, Vn, Gn, None, True, True)
    eng = next(iter(torch_op._cache.values())).eng
    assert eng.last_kernel() == "attention_fused_backward+long_rows"
    want = reference(rp, ci, v, M, K, Qn, Kn, Vn, Gn, 0.25, True)
    check(got, want, True)
    ones = np.flatnonzero(np.diff(rp) == 1)   # a row of one entry: p = 1, O is V's row
    assert len(ones) == 2101
    assert same(got[0][ones], Vn[ci[rp[ones]]])
    # the forward alone names its own kernel
    import torch
    A = make_A(rp, ci, v, M, K)
    torch_op.sparse_attention(A, *(torch.from_numpy(t).cuda() for t in (Qn, Kn, Vn)), fused=True)
    assert list(torch_op._cache.values())[-1].eng.last_kernel() == "attention_fused+long_rows"   # (A's new index tensors: a new entry)
    torch_op.clear_cache()


class Abi:
    """one engine on a pattern, operands as torch tensors, the two entry points called through api.Engine"""

    def __init__(self, sx, rp, ci, M, K, H, d, dv):
        import torch
        self.t = torch
        self.M, self.K, self.H, self.d, self.dv, self.nnz = M, K, H, d, dv, len(ci)
        self.rp, self.ci = torch.from_numpy(rp.astype(np.int32)).cuda(), torch.from_numpy(ci.astype(np.int32)).cuda()
        self.val = torch.full((max(len(ci), 1),), float("nan"), device="cuda")   # A's own values are not read
        self.eng = sx.Engine(0)
        self.eng.set_matrix_csr_device(M, K, len(ci), self.rp.data_ptr(), self.ci.data_ptr(), self.val.data_ptr())

    def forward(self, Q, Kt, V, bias, scale):
        t, H, d, dv = self.t, self.H, self.d, self.dv
        O = t.full((self.M, H, dv), 7.0, device="cuda"); lse = t.full((self.M, H), 7.0, device="cuda")
        self.eng.attention_device(H, d, dv, scale, Q.data_ptr(), H * d, Kt.data_ptr(), H * d, V.data_ptr(), H * dv,
                                  bias.data_ptr() if bias is not None else None, O.data_ptr(), H * dv, lse.data_ptr(),
                                  t.cuda.current_stream().cuda_stream)
        return O, lse

    def backward(self, Q, Kt, V, bias, scale, O, lse, G, want_dbias=True):
        t, H, d, dv = self.t, self.H, self.d, self.dv
        delta = t.full((self.M, H), 7.0, device="cuda")
        dQ, dK, dV = t.full((self.M, H, d), 7.0, device="cuda"), t.full((self.K, H, d), 7.0, device="cuda"), t.full((self.K, H, dv), 7.0, device="cuda")
        db = t.full((max(self.nnz, 1),), 7.0, device="cuda") if want_dbias else None
        self.eng.attention_backward_device(H, d, dv, scale, Q.data_ptr(), H * d, Kt.data_ptr(), H * d, V.data_ptr(), H * dv,
                                           bias.data_ptr() if bias is not None else None, O.data_ptr(), H * dv, lse.data_ptr(), G.data_ptr(), H * dv,
                                           delta.data_ptr(), dQ.data_ptr(), H * d, dK.data_ptr(), H * d, dV.data_ptr(), H * dv,
                                           db.data_ptr() if db is not None else None, t.cuda.current_stream().cuda_stream)
        return dQ, dK, dV, (db[:self.nnz] if db is not None else None)


def test_empty_rows_and_masks_on_the_c_abi(sx):
    import torch
    from util import random_csr
    rs = np.random.RandomState(17)
    M, K, H, d, dv, scale = 400, 400, 2, 16, 24, 0.3
    rp, ci, _ = random_csr(rs, M, K - 20, 6, empty_frac=0.2)   # the last 20 columns have no entry
    lens = np.diff(rp)
    empty = np.flatnonzero(lens == 0)
    assert len(empty) > 20
    nnz = len(ci)
    Q, Kt, V, G = (torch.from_numpy(rand(rs, n, H, w)).cuda() for n, w in ((M, d), (K, d), (K, dv), (M, dv)))
    bias_n = rand(rs, nnz)
    # rows of two or more entries: their first entry is masked out (-inf); one row of three is masked out completely
    multi = np.flatnonzero(lens >= 2)
    dead = int(np.flatnonzero(lens == 3)[0])
    masked = rp[multi[multi != dead]]
    bias_n[masked] = -np.inf
    bias_n[rp[dead]:rp[dead + 1]] = -np.inf
    bias = torch.from_numpy(bias_n).cuda()
    a = Abi(sx, rp, ci, M, K, H, d, dv)
    O, lse = a.forward(Q, Kt, V, bias, scale)
    dQ, dK, dV, db = a.backward(Q, Kt, V, bias, scale, O, lse, G)
    assert a.eng.last_kernel() == "attention_fused_backward"
    On, lsen, dQn, dKn, dVn, dbn = (x.cpu().numpy() for x in (O, lse, dQ, dK, dV, db))
    # empty rows: O = +0 (the bits), lse = -inf, dQ = 0; columns without entries: dK = dV = 0
    assert np.all(On[empty].view(np.uint32) == 0) and np.all(lsen[empty] == -np.inf) and np.all(dQn[empty] == 0)
    assert np.all(dKn[K - 20:] == 0) and np.all(dVn[K - 20:] == 0)
    # the row whose scores are all -inf is NaN in every head, and nothing else is
    alive = np.ones(M, bool); alive[dead] = False
    assert np.all(np.isnan(On[dead])) and np.all(np.isfinite(On[alive])) and np.all(np.isfinite(dQn[alive]))
    assert np.all(np.isfinite(lsen[alive & (lens > 0)]))
    # a -inf entry beside finite ones contributes exactly 0: the results of the pattern without those entries (and without the dead row's)
    assert np.all(dbn[masked] == 0)
    keep = np.ones(nnz, bool); keep[masked] = False; keep[rp[dead]:rp[dead + 1]] = False
    rows = np.repeat(np.arange(M), lens)
    rp2 = np.zeros(M + 1, np.int32); rp2[1:] = np.cumsum(np.bincount(rows[keep], minlength=M))
    b = Abi(sx, rp2, ci[keep], M, K, H, d, dv)
    bias2 = torch.from_numpy(bias_n[keep]).cuda()
    O2, lse2 = b.forward(Q, Kt, V, bias2, scale)
    dQ2, dK2, dV2, db2 = b.backward(Q, Kt, V, bias2, scale, O2, lse2, G)
    O2n, dQ2n, dK2n, dV2n, db2n = (x.cpu().numpy() for x in (O2, dQ2, dK2, dV2, db2))
    assert np.all(O2n[dead] == 0) and _close(On[alive], O2n[alive]) and _close(lsen[alive & (lens > 0)], lse2.cpu().numpy()[alive & (lens > 0)])
    assert _close(dQn[alive], dQ2n[alive]) and _close(dbn[keep], db2n)
    # (the dead row's NaN reaches the dK / dV rows of its columns: compare the others -- they are most)
    clean = np.ones(K, bool); clean[ci[rp[dead]:rp[dead + 1]]] = False
    assert clean.mean() >= 0.99
    assert np.all(np.isfinite(dKn[clean])) and _close(dKn[clean], dK2n[clean]) and _close(dVn[clean], dV2n[clean])
    # a NULL operand with nnz > 0 is refused; without bias and dbias the call is complete
    with pytest.raises(sx.api.SextansError) as err:
        a.eng.attention_device(H, d, dv, scale, Q.data_ptr(), H * d, None, H * d, V.data_ptr(), H * dv, None, O.data_ptr(), H * dv, lse.data_ptr(), None)
    assert err.value.code == INVALID
    O3, lse3 = a.forward(Q, Kt, V, None, scale)
    dQ3 = a.backward(Q, Kt, V, None, scale, O3, lse3, G, want_dbias=False)[0]
    assert np.all(np.isfinite(O3.cpu().numpy())) and np.all(np.isfinite(dQ3.cpu().numpy()))
    # no entries at all: everything is written, nothing is launched on the pattern
    c = Abi(sx, np.zeros(M + 1, np.int32), np.zeros(0, np.int32), M, K, H, d, dv)
    O4, lse4 = c.forward(Q, Kt, V, None, scale)
    dQ4, dK4, dV4, _ = c.backward(Q, Kt, V, None, scale, O4, lse4, G, want_dbias=False)
    assert np.all(O4.cpu().numpy().view(np.uint32) == 0) and np.all(lse4.cpu().numpy() == -np.inf)
    assert all(np.all(x.cpu().numpy() == 0) for x in (dQ4, dK4, dV4))
    for e in (a, b, c):
        e.eng.close()


def test_agrees_with_the_composition(sx):
    import torch
    from sextans_amd import torch_op
    M, K, H, d, dv = 500, 420, 3, 16, 32
    rs, rp, ci, v = pattern(41, M, K, 11)
    Qn, Kn, Vn, Gn = rand(rs, M, H, d), rand(rs, K, H, d), rand(rs, K, H, dv), rand(rs, M, H, dv)
    torch_op.clear_cache()
    fused = run(rp, ci, v, M, K, Qn, Kn, Vn, Gn, None, True, True)
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0, info
    torch_op.clear_cache()
    comp = run(rp, ci, v, M, K, Qn, Kn, Vn, Gn, None, True, False)
    assert torch_op.cache_info()["value_refreshes"] > 0
    for g, w, name in zip(fused, comp, ("O", "dQ", "dK", "dV", "dA")):
        assert _close(g, w), name
    # heads through the composition = the 2-D calls, stacked
    A = make_A(rp, ci, v, M, K)
    Q, Kt, V = (torch.from_numpy(t).cuda() for t in (Qn, Kn, Vn))
    with torch.no_grad():
        stacked = torch.stack([torch_op.sparse_attention(A, Q[:, h], Kt[:, h], V[:, h], bias=True) for h in range(H)], dim=1)
        whole = torch_op.sparse_attention(A, Q, Kt, V, bias=True)
    assert same(whole.cpu().numpy(), stacked.cpu().numpy()) and same(whole.cpu().numpy(), comp[0])
    torch_op.clear_cache()


def test_determinism_and_captured_training_step(sx):
    """forward, backward and an SGD update of Q, K and V in place, captured once (refresh(A) outside the capture first) and replayed three
    times: bit for bit three eager steps, on one engine."""
    import torch
    from sextans_amd import torch_op
    M, K, H, d = 900, 900, 2, 16
    rs, rp, ci, v = pattern(21, M, K, 10)
    Qn, Kn, Vn, Gn = (rand(rs, n, H, d) for n in (M, K, K, M))
    G = torch.from_numpy(Gn).cuda()
    torch_op.clear_cache()
    first = run(rp, ci, v, M, K, Qn, Kn, Vn, Gn, None, True, True)
    second = run(rp, ci, v, M, K, Qn, Kn, Vn, Gn, None, True, True)
    for x, y in zip(first, second):
        assert same(x, y)

    def start():
        A = make_A(rp, ci, v, M, K)
        with torch.no_grad():
            A.values().mul_(0.5)          # (in place: moves the version counter of A's index tensors too)
        return A, [torch.from_numpy(t).cuda().requires_grad_() for t in (Qn, Kn, Vn)]

    def step(A, params):
        for t in params:
            t.grad = None
        out = torch_op.sparse_attention(A, *params, bias=True, fused=True)
        out.backward(G)
        with torch.no_grad():
            for t in params:
                t.sub_(LR * t.grad)
        return out

    def state(out, params):
        return [out.detach().cpu().numpy().copy()] + [t.detach().cpu().numpy().copy() for t in params]

    torch_op.clear_cache()
    A, params = start()
    eager = [state(step(A, params), params) for _ in range(4)]
    assert not np.array_equal(eager[3][1], eager[0][1])
    torch_op.clear_cache()
    A, params = start()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(A, params)                   # warm-up: engine, softmax tables, A^T and its tables
        torch_op.refresh(A)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step(A, params)
    assert torch_op.cache_info()["engines_built"] == 1
    for k in range(1, 4):
        g.replay()
        torch.cuda.synchronize()
        got = state(out, params)
        for i in range(4):
            assert same(got[i], eager[k][i]), (k, i)
    torch_op.clear_cache()


def test_operand_placement(sx):
    import torch
    from sextans_amd import torch_op
    M, K, H, d, dv = 260, 240, 2, 16, 24
    rs, rp, ci, v = pattern(51, M, K, 8)
    Qn, Kn, Vn, Gn = rand(rs, M, H, d), rand(rs, K, H, d), rand(rs, K, H, dv), rand(rs, M, H, dv)
    torch_op.clear_cache()
    base = run(rp, ci, v, M, K, Qn, Kn, Vn, Gn, None, False, True)

    def outcome(Q, Kt, V):
        A = make_A(rp, ci, v, M, K)
        out = torch_op.sparse_attention(A, Q, Kt, V, fused=True)
        out.backward(torch.from_numpy(Gn).cuda())
        return [t.detach().cpu().numpy() for t in (out, Q.grad, Kt.grad, V.grad)]

    def in_wider_buffer(t, pad, off):
        """(rows, H, w) as columns [off, off + H w) of a (rows, H w + pad) buffer: a leaf the kernels read where it lies"""
        rows, h, w = t.shape
        buf = torch.full((rows, h * w + pad), 9.0, device="cuda")
        view = buf[:, off:off + h * w].unflatten(1, (h, w))
        view.copy_(torch.from_numpy(t))
        assert view.stride(0) > h * w and view.data_ptr() % 16 == 0 and not view.is_contiguous()
        return view.detach().requires_grad_()

    got = outcome(in_wider_buffer(Qn, 8, 4), in_wider_buffer(Kn, 16, 8), in_wider_buffer(Vn, 4, 0))
    for x, y in zip(got, base):
        assert same(x, y)
    # a V the kernels cannot read where it lies (heads not side by side) is copied
    Vt = torch.from_numpy(np.ascontiguousarray(Vn.transpose(1, 0, 2))).cuda().transpose(0, 1).requires_grad_()
    assert not Vt.is_contiguous() and Vt.stride(1) != dv
    Q, Kt = (torch.from_numpy(t).cuda().requires_grad_() for t in (Qn, Kn))
    got = outcome(Q, Kt, Vt)
    for x, y in zip(got, base):
        assert same(x, y)
    torch_op.clear_cache()


def test_errors(sx):
    import torch
    from sextans_amd import torch_op
    M, K = 60, 50
    rs, rp, ci, v = pattern(2, M, K, 4)
    A = make_A(rp, ci, v, M, K)
    z = lambda *s: torch.zeros(*s, device="cuda")   # noqa: E731
    for fused in (False, True):
        with pytest.raises(ValueError):
            torch_op.sparse_attention(A, z(M, 2, 16), z(K, 3, 16), z(K, 2, 16), fused=fused)    # heads
        with pytest.raises(ValueError):
            torch_op.sparse_attention(A, z(M, 2, 16), z(K, 2, 16), z(K, 1, 16), fused=fused)
        with pytest.raises(ValueError):
            torch_op.sparse_attention(A, z(M, 2, 16), z(K, 2, 8), z(K, 2, 16), fused=fused)     # d
        with pytest.raises(ValueError):
            torch_op.sparse_attention(A, z(M, 2, 16), z(K, 2, 16), z(K - 1, 2, 16), fused=fused)
        with pytest.raises(TypeError):
            torch_op.sparse_attention(A, z(M, 2, 16).cpu(), z(K, 2, 16), z(K, 2, 16), fused=fused)
        with pytest.raises(TypeError):
            torch_op.sparse_attention(A.cpu(), z(M, 2, 16), z(K, 2, 16), z(K, 2, 16), fused=fused)
    with pytest.raises(ValueError):
        torch_op.sparse_attention(A, z(M, 1, 136), z(K, 1, 136), z(K, 1, 16), fused=True)
    with pytest.raises(ValueError):
        torch_op.sparse_attention(A, z(M, 16), z(K, 16), z(K, 136), fused=True)
    torch_op.clear_cache()
