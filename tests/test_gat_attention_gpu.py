"""gat_attention and the C ABI under it (sextans_gat_attention_device, sextans_gat_attention_backward_device): graph attention with the
additive score leaky_relu(a_dst[r] + a_src[c] (+ A_e)) in one kernel pass per direction, against the float64 dense masked computation per
head (forward and every gradient) with the tolerance the fused dot-product attention is held to (test_torch_autograd_gpu._close, rtol
2e-4); row lengths around every lane-group size and beyond the long-row threshold; empty rows, unused columns and -inf masks at slopes 0.2
and 0; agreement with the dot-product kernel when the activation is the identity; bit-reproducibility and a captured training step;
operands read where they lie.  The derivative of LeakyReLU jumps at 0: every test that compares gradients first asserts, on the CPU,
that the float64 |z| of every stored entry exceeds 1e-5."""
import numpy as np
import pytest

from test_fused_attention_gpu import edge_pattern, rand, same
from test_torch_attention_gpu import make_A, pattern
from test_torch_autograd_gpu import _close

pytestmark = pytest.mark.gpu

LR = 0.05
INVALID = 9


def assert_off_the_kink(rp, ci, adn, asn, bias_values=None):
    """float64 z = a_dst[r, h] + a_src[c, h] (+ bias_e) of every stored entry and head stays away from LeakyReLU's kink"""
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    z = adn.astype(np.float64)[rows] + asn.astype(np.float64)[ci]
    if bias_values is not None:
        z = z + bias_values.astype(np.float64)[:, None]
    assert np.all(np.abs(z) > 1e-5), float(np.abs(z).min())


def reference(rp, ci, v, M, K, adn, asn, Vn, Gn, slope, bias):
    """float64 dense masked graph attention head by head: O (M, H, dv), d a_dst (M, H), d a_src (K, H), dV and the bias gradient summed
    over the heads"""
    import torch
    H = Vn.shape[1]
    rows = torch.from_numpy(np.repeat(np.arange(M), np.diff(rp))).cuda()
    cols = torch.from_numpy(ci.astype(np.int64)).cuda()
    mask = torch.full((M, K), float("-inf"), dtype=torch.float64, device="cuda")
    mask[rows, cols] = 0.0
    out = {k: [] for k in ("O", "dad", "das", "dV")}
    dA = 0.0
    for h in range(H):
        ad, as_, V = (torch.from_numpy(np.ascontiguousarray(t[:, h])).cuda().double().requires_grad_() for t in (adn, asn, Vn))
        Av = torch.from_numpy(v).cuda().double().requires_grad_()
        Z = ad[:, None] + as_[None, :]
        if bias:
            Z = Z + torch.zeros((M, K), dtype=torch.float64, device="cuda").index_put((rows, cols), Av)
        P = torch.softmax(torch.nn.functional.leaky_relu(Z, slope) + mask, dim=1)
        O = P @ V
        O.backward(torch.from_numpy(np.ascontiguousarray(Gn[:, h])).cuda().double())
        out["O"].append(O.detach().cpu().numpy())
        out["dad"].append(ad.grad.cpu().numpy()); out["das"].append(as_.grad.cpu().numpy()); out["dV"].append(V.grad.cpu().numpy())
        if bias:
            dA = dA + Av.grad.cpu().numpy()
    res = {k: np.stack(x, axis=1) for k, x in out.items()}
    res["dA"] = dA
    return res


def run(rp, ci, v, M, K, adn, asn, Vn, Gn, slope, bias, squeeze=False):
    """-> (O, d a_dst, d a_src, dV, dA values or None) as numpy, heads on axis 1; squeeze: hand H = 1 operands over as (rows,) and (rows, dv)"""
    import torch
    from sextans_amd import torch_op
    A = make_A(rp, ci, v, M, K, grad=bias)
    ad, as_, V = (torch.from_numpy(t[:, 0] if squeeze else t).cuda().requires_grad_() for t in (adn, asn, Vn))
    out = torch_op.gat_attention(A, ad, as_, V, negative_slope=slope, bias=bias)
    assert out.dim() == V.dim()
    out.backward(torch.from_numpy(Gn[:, 0] if squeeze else Gn).cuda())
    if bias:
        assert A.grad.layout == torch.sparse_csr and A.grad.values().dtype == A.values().dtype
    else:
        assert A.grad is None
    assert ad.grad.shape == ad.shape and as_.grad.shape == as_.shape and ad.grad.dtype == ad.dtype
    res = [t.detach().cpu().numpy() for t in (out, ad.grad, as_.grad, V.grad)]
    if squeeze:
        res = [t[:, None] for t in res]
    return res + [A.grad.values().cpu().numpy() if bias else None]


def check(got, want, bias):
    for g, k in zip(got, ("O", "dad", "das", "dV")):
        assert g.shape == want[k].shape, k
        assert np.all(np.isfinite(g)), k
        assert _close(g, want[k]), (k, float(np.abs(g - want[k]).max()))
    if bias:
        assert _close(got[4], want["dA"]), ("dA", float(np.abs(got[4] - want["dA"]).max()))


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("H, dv, slope", [(1, 16, 0.2), (3, 24, 0.2), (2, 64, 0.2), (2, 40, 0.2), (1, 128, 0.2), (3, 24, 0.0)])
def test_against_dense_float64(sx, H, dv, slope, bias):
    from sextans_amd import torch_op
    M, K = 300, 260
    rs, rp, ci, v = pattern(31 + dv, M, K, 9)
    assert np.all(np.diff(rp) > 0)
    adn, asn, Vn, Gn = rand(rs, M, H), rand(rs, K, H), rand(rs, K, H, dv), rand(rs, M, H, dv)
    assert_off_the_kink(rp, ci, adn, asn, v if bias else None)
    torch_op.clear_cache()
    got = run(rp, ci, v, M, K, adn, asn, Vn, Gn, slope, bias, squeeze=(H == 1 and dv == 16))
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0, info
    want = reference(rp, ci, v, M, K, adn, asn, Vn, Gn, slope, bias)
    check(got, want, bias)
    torch_op.clear_cache()


def test_row_length_edges_and_long_rows(sx):
    import torch
    from sextans_amd import torch_op
    rs = np.random.RandomState(8)
    rp, ci, v, M, K = edge_pattern(rs)
    assert M < 3000 and np.count_nonzero(ci == 0) > 2048 and np.diff(rp).max() == 2500
    H, dv = 2, 16
    adn, asn, Vn, Gn = rand(rs, M, H), rand(rs, K, H), rand(rs, K, H, dv), rand(rs, M, H, dv)
    assert_off_the_kink(rp, ci, adn, asn, v)
    torch_op.clear_cache()
    got = run(rp, ci, v, M, K, adn, asn, Vn, Gn, 0.2, True)
    eng = next(iter(torch_op._cache.values())).eng
    assert eng.last_kernel() == "gat_fused_backward+long_rows"
    want = reference(rp, ci, v, M, K, adn, asn, Vn, Gn, 0.2, True)
    check(got, want, True)
    ones = np.flatnonzero(np.diff(rp) == 1)   # a row of one entry: p = 1, O is V's row
    assert len(ones) == 2101
    assert same(got[0][ones], Vn[ci[rp[ones]]])
    # the forward alone names its own kernel
    A = make_A(rp, ci, v, M, K)
    torch_op.gat_attention(A, *(torch.from_numpy(t).cuda() for t in (adn, asn, Vn)))
    assert list(torch_op._cache.values())[-1].eng.last_kernel() == "gat_fused+long_rows"   # (A's new index tensors: a new entry)
    torch_op.clear_cache()


class Abi:
    """one engine on a pattern, operands as torch tensors, the two entry points called through api.Engine"""

    def __init__(self, sx, rp, ci, M, K, H, dv):
        import torch
        self.t = torch
        self.M, self.K, self.H, self.dv, self.nnz = M, K, H, dv, len(ci)
        self.rp, self.ci = torch.from_numpy(rp.astype(np.int32)).cuda(), torch.from_numpy(ci.astype(np.int32)).cuda()
        self.val = torch.full((max(len(ci), 1),), float("nan"), device="cuda")   # A's own values are not read
        self.eng = sx.Engine(0)
        self.eng.set_matrix_csr_device(M, K, len(ci), self.rp.data_ptr(), self.ci.data_ptr(), self.val.data_ptr())

    def forward(self, ad, as_, V, bias, slope):
        t, H, dv = self.t, self.H, self.dv
        O = t.full((self.M, H, dv), 7.0, device="cuda"); lse = t.full((self.M, H), 7.0, device="cuda")
        self.eng.gat_attention_device(H, dv, slope, ad.data_ptr(), H, as_.data_ptr(), H, V.data_ptr(), H * dv,
                                      bias.data_ptr() if bias is not None else None, O.data_ptr(), H * dv, lse.data_ptr(),
                                      t.cuda.current_stream().cuda_stream)
        return O, lse

    def backward(self, ad, as_, V, bias, slope, O, lse, G, want_dbias=True):
        t, H, dv = self.t, self.H, self.dv
        delta = t.full((self.M, H), 7.0, device="cuda")
        dad, das, dV = t.full((self.M, H), 7.0, device="cuda"), t.full((self.K, H), 7.0, device="cuda"), t.full((self.K, H, dv), 7.0, device="cuda")
        db = t.full((max(self.nnz, 1),), 7.0, device="cuda") if want_dbias else None
        self.eng.gat_attention_backward_device(H, dv, slope, ad.data_ptr(), H, as_.data_ptr(), H, V.data_ptr(), H * dv,
                                               bias.data_ptr() if bias is not None else None, O.data_ptr(), H * dv, lse.data_ptr(), G.data_ptr(),
                                               H * dv, delta.data_ptr(), dad.data_ptr(), H, das.data_ptr(), H, dV.data_ptr(), H * dv,
                                               db.data_ptr() if db is not None else None, t.cuda.current_stream().cuda_stream)
        self.delta = delta
        return dad, das, dV, (db[:self.nnz] if db is not None else None)


@pytest.mark.parametrize("slope", [0.2, 0.0])
def test_empty_rows_and_masks_on_the_c_abi(sx, slope):
    import torch
    from util import random_csr
    rs = np.random.RandomState(17)
    M, K, H, dv = 400, 400, 2, 24
    rp, ci, _ = random_csr(rs, M, K - 20, 6, empty_frac=0.2)   # the last 20 columns have no entry
    lens = np.diff(rp)
    empty = np.flatnonzero(lens == 0)
    assert len(empty) > 20
    nnz = len(ci)
    adn, asn, Vn, Gn = rand(rs, M, H), rand(rs, K, H), rand(rs, K, H, dv), rand(rs, M, H, dv)
    bias_n = rand(rs, nnz)
    # rows of two or more entries: their first entry is masked out (-inf); one row of three is masked out completely
    multi = np.flatnonzero(lens >= 2)
    dead = int(np.flatnonzero(lens == 3)[0])
    masked = rp[multi[multi != dead]]
    bias_n[masked] = -np.inf
    bias_n[rp[dead]:rp[dead + 1]] = -np.inf
    assert_off_the_kink(rp, ci, adn, asn, bias_n)   # (a masked entry: |z| = inf)
    ad, as_, V, G = (torch.from_numpy(t).cuda() for t in (adn, asn, Vn, Gn))
    bias = torch.from_numpy(bias_n).cuda()
    a = Abi(sx, rp, ci, M, K, H, dv)
    O, lse = a.forward(ad, as_, V, bias, slope)
    dad, das, dV, db = a.backward(ad, as_, V, bias, slope, O, lse, G)
    assert a.eng.last_kernel() == "gat_fused_backward"
    On, lsen, dadn, dasn, dVn, dbn = (x.cpu().numpy() for x in (O, lse, dad, das, dV, db))
    # empty rows: O = +0 (the bits), lse = -inf, d a_dst = 0; columns without entries: d a_src = dV = 0
    assert np.all(On[empty].view(np.uint32) == 0) and np.all(lsen[empty] == -np.inf) and np.all(dadn[empty] == 0)
    assert np.all(dasn[K - 20:] == 0) and np.all(dVn[K - 20:] == 0)
    # the row whose scores are all -inf is NaN in every head, and nothing else is: the -inf masks also at slope 0
    alive = np.ones(M, bool); alive[dead] = False
    assert np.all(np.isnan(On[dead])) and np.all(np.isfinite(On[alive])) and np.all(np.isfinite(dadn[alive]))
    assert np.all(np.isnan(dadn[dead])) and np.all(np.isnan(dbn[rp[dead]:rp[dead + 1]]))
    assert np.all(np.isfinite(lsen[alive & (lens > 0)]))
    # a -inf entry beside finite ones contributes exactly 0: the results of the pattern without those entries (and without the dead row's)
    assert np.all(dbn[masked] == 0)
    keep = np.ones(nnz, bool); keep[masked] = False; keep[rp[dead]:rp[dead + 1]] = False
    rows = np.repeat(np.arange(M), lens)
    rp2 = np.zeros(M + 1, np.int32); rp2[1:] = np.cumsum(np.bincount(rows[keep], minlength=M))
    b = Abi(sx, rp2, ci[keep], M, K, H, dv)
    bias2 = torch.from_numpy(bias_n[keep]).cuda()
    O2, lse2 = b.forward(ad, as_, V, bias2, slope)
    dad2, das2, dV2, db2 = b.backward(ad, as_, V, bias2, slope, O2, lse2, G)
    O2n, dad2n, das2n, dV2n, db2n = (x.cpu().numpy() for x in (O2, dad2, das2, dV2, db2))
    assert np.all(O2n[dead] == 0) and _close(On[alive], O2n[alive]) and _close(lsen[alive & (lens > 0)], lse2.cpu().numpy()[alive & (lens > 0)])
    assert _close(dadn[alive], dad2n[alive]) and _close(dbn[keep], db2n)
    # (the dead row's NaN reaches the d a_src / dV rows of its columns: compare the others -- they are most)
    clean = np.ones(K, bool); clean[ci[rp[dead]:rp[dead + 1]]] = False
    assert clean.mean() >= 0.99
    assert np.all(np.isfinite(dasn[clean])) and np.all(np.isfinite(dVn[clean]))
    assert _close(dasn[clean], das2n[clean]) and _close(dVn[clean], dV2n[clean])
    # a NULL operand with nnz > 0 is refused; without bias and dbias the call is complete
    with pytest.raises(sx.api.SextansError) as err:
        a.eng.gat_attention_device(H, dv, slope, ad.data_ptr(), H, as_.data_ptr(), H, None, H * dv, None, O.data_ptr(), H * dv, lse.data_ptr(), None)
    assert err.value.code == INVALID
    O3, lse3 = a.forward(ad, as_, V, None, slope)
    dad3 = a.backward(ad, as_, V, None, slope, O3, lse3, G, want_dbias=False)[0]
    assert np.all(np.isfinite(O3.cpu().numpy())) and np.all(np.isfinite(dad3.cpu().numpy()))
    # no entries at all: everything is written, nothing is launched on the pattern
    c = Abi(sx, np.zeros(M + 1, np.int32), np.zeros(0, np.int32), M, K, H, dv)
    O4, lse4 = c.forward(ad, as_, V, None, slope)
    dad4, das4, dV4, _ = c.backward(ad, as_, V, None, slope, O4, lse4, G, want_dbias=False)
    assert np.all(O4.cpu().numpy().view(np.uint32) == 0) and np.all(lse4.cpu().numpy() == -np.inf)
    assert all(np.all(x.cpu().numpy() == 0) for x in (dad4, das4, dV4, c.delta))
    for e in (a, b, c):
        e.eng.close()


def test_identity_activation_equals_the_dot_product_kernel(sx):
    """slope 1: the activation is the identity, and the additive score is the dot product of Q = (a_dst, 1, 0, ..) and K = (1, a_src, 0, ..).
    (At slope 1, d a_dst is the sum of ds over a softmax row: zero but for rounding.  The comparison with dQ[..., 0] holds because the
    two forward kernels form the same batches and the two row passes add in the same order, so the same roundings are made.)"""
    import torch
    from sextans_amd import torch_op
    M, K, H, dv, d = 500, 420, 3, 32, 8
    rs, rp, ci, v = pattern(41, M, K, 11)
    adn, asn, Vn, Gn = rand(rs, M, H), rand(rs, K, H), rand(rs, K, H, dv), rand(rs, M, H, dv)
    assert_off_the_kink(rp, ci, adn, asn)
    Qn, Kn = np.zeros((M, H, d), np.float32), np.zeros((K, H, d), np.float32)
    Qn[:, :, 0] = adn; Qn[:, :, 1] = 1.0
    Kn[:, :, 0] = 1.0; Kn[:, :, 1] = asn
    G = torch.from_numpy(Gn).cuda()
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    ad, as_, V = (torch.from_numpy(t).cuda().requires_grad_() for t in (adn, asn, Vn))
    out = torch_op.gat_attention(A, ad, as_, V, negative_slope=1.0)
    out.backward(G)
    Q, Kt, V2 = (torch.from_numpy(t).cuda().requires_grad_() for t in (Qn, Kn, Vn))
    ref = torch_op.sparse_attention(A, Q, Kt, V2, scale=1.0, fused=True)
    ref.backward(G)
    assert torch_op.cache_info()["engines_built"] == 1
    n = lambda t: t.detach().cpu().numpy()   # noqa: E731
    assert _close(n(out), n(ref)) and _close(n(V.grad), n(V2.grad))
    assert _close(n(ad.grad), n(Q.grad)[..., 0]) and _close(n(as_.grad), n(Kt.grad)[..., 1])
    torch_op.clear_cache()


def test_determinism_and_captured_training_step(sx):
    """forward, backward and an SGD update of a_dst, a_src and V in place, captured once (refresh(A) outside the capture first) and
    replayed three times: bit for bit three eager steps, on one engine."""
    import torch
    from sextans_amd import torch_op
    M, K, H, dv = 900, 900, 2, 16
    rs, rp, ci, v = pattern(21, M, K, 10)
    adn, asn, Vn, Gn = rand(rs, M, H), rand(rs, K, H), rand(rs, K, H, dv), rand(rs, M, H, dv)
    assert_off_the_kink(rp, ci, adn, asn, v)
    G = torch.from_numpy(Gn).cuda()
    torch_op.clear_cache()
    first = run(rp, ci, v, M, K, adn, asn, Vn, Gn, 0.2, True)
    second = run(rp, ci, v, M, K, adn, asn, Vn, Gn, 0.2, True)
    for x, y in zip(first, second):
        assert same(x, y)

    def start():
        A = make_A(rp, ci, v, M, K)
        with torch.no_grad():
            A.values().mul_(0.5)          # (in place: moves the version counter of A's index tensors too)
        return A, [torch.from_numpy(t).cuda().requires_grad_() for t in (adn, asn, Vn)]

    def step(A, params):
        for t in params:
            t.grad = None
        out = torch_op.gat_attention(A, *params, bias=True)
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
    M, K, H, dv = 260, 240, 2, 24
    rs, rp, ci, v = pattern(51, M, K, 8)
    adn, asn, Vn, Gn = rand(rs, M, H), rand(rs, K, H), rand(rs, K, H, dv), rand(rs, M, H, dv)
    torch_op.clear_cache()
    base = run(rp, ci, v, M, K, adn, asn, Vn, Gn, 0.2, False)[:4]

    def outcome(ad, as_, V):
        A = make_A(rp, ci, v, M, K)
        out = torch_op.gat_attention(A, ad, as_, V)
        out.backward(torch.from_numpy(Gn).cuda())
        return [t.detach().cpu().numpy() for t in (out, ad.grad, as_.grad, V.grad)]

    def in_wider_buffer(t, pad, off):
        """(rows, H, w) or (rows, H) as columns [off, off + H w) of a (rows, H w + pad) buffer: a leaf the kernels read where it lies"""
        rows, h = t.shape[:2]
        w = t.shape[2] if t.ndim == 3 else 1
        buf = torch.full((rows, h * w + pad), 9.0, device="cuda")
        view = buf[:, off:off + h * w]
        if t.ndim == 3:
            view = view.unflatten(1, (h, w))
        view.copy_(torch.from_numpy(t))
        assert view.stride(0) > h * w and view.data_ptr() % 16 == 0 and not view.is_contiguous()
        return view.detach().requires_grad_()

    from sextans_amd.torch_op import _heads_operand, _scalars_operand
    wide = [in_wider_buffer(adn, 6, 4), in_wider_buffer(asn, 10, 8), in_wider_buffer(Vn, 4, 0)]
    assert _scalars_operand(wide[0])[0] is wide[0] and _scalars_operand(wide[1])[0] is wide[1] and _heads_operand(wide[2], dv)[0] is wide[2]
    got = outcome(*wide)
    for x, y in zip(got, base):
        assert same(x, y)
    # a V the kernels cannot read where it lies (heads not side by side) is copied
    Vt = torch.from_numpy(np.ascontiguousarray(Vn.transpose(1, 0, 2))).cuda().transpose(0, 1).requires_grad_()
    assert not Vt.is_contiguous() and Vt.stride(1) != dv and _heads_operand(Vt.detach(), dv)[0] is not Vt
    ad, as_ = (torch.from_numpy(t).cuda().requires_grad_() for t in (adn, asn))
    got = outcome(ad, as_, Vt)
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
    with pytest.raises(ValueError):
        torch_op.gat_attention(A, z(M, 3), z(K, 2), z(K, 2, 16))        # heads
    with pytest.raises(ValueError):
        torch_op.gat_attention(A, z(M, 2), z(K, 1), z(K, 2, 16))
    with pytest.raises(ValueError):
        torch_op.gat_attention(A, z(M), z(K), z(K, 2, 16))
    with pytest.raises(ValueError):
        torch_op.gat_attention(A, z(M - 1, 2), z(K, 2), z(K, 2, 16))    # rows
    with pytest.raises(ValueError):
        torch_op.gat_attention(A, z(M, 2), z(K, 2), z(K - 1, 2, 16))
    with pytest.raises(ValueError):
        torch_op.gat_attention(A, z(M, 2), z(M, 2), z(K, 2, 16))
    with pytest.raises(ValueError):
        torch_op.gat_attention(A, z(M), z(K), z(K, 136))                # dv
    with pytest.raises(ValueError):
        torch_op.gat_attention(A, z(M, 1), z(K, 1), z(K, 1, 136))
    with pytest.raises(TypeError):
        torch_op.gat_attention(A, z(M, 2).cpu(), z(K, 2), z(K, 2, 16))
    with pytest.raises(TypeError):
        torch_op.gat_attention(A, z(M, 2), z(K, 2), z(K, 2, 16).cpu())
    with pytest.raises(TypeError):
        torch_op.gat_attention(A.cpu(), z(M, 2), z(K, 2), z(K, 2, 16))
    torch_op.clear_cache()
