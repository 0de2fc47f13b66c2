"""gatv2_attention and the C ABI under it (sextans_gatv2_attention_device, sextans_gatv2_attention_backward_device): GATv2's score
<att, leaky_relu(x_dst[r] + x_src[c])> (+ A_e) with x_src as the message, in one kernel pass per direction, against a float64 computation
on the edge list (forward and every gradient, torch autograd) with the tolerance the fused dot-product attention and GAT are held to
(test_torch_autograd_gpu._close, rtol 2e-4); row lengths around every lane-group size and beyond the long-row threshold; the forward's
bits against the GAT kernel when att picks one feature; the fixed order of att's gradient, recomputed add by add; bit-reproducibility
and a captured training step; empty rows, unused columns, -inf masks, patterns without entries or rows; shared weights; operands read
where they lie.
The derivative of LeakyReLU jumps at 0 and every entry now has H * d values of z.  The features of every gradient comparison lie on a
grid -- x_dst = i / 32, x_src = (j + 1/2) / 32 with integers i, j in [-32, 32] -- so that z = (i + j + 1/2) / 32 is exact in fp32 and
|z| >= 1 / 64; each such test still asserts, on the CPU, that the float64 |z| of every (entry, head, k) exceeds 1e-5."""
import numpy as np
import pytest

from test_fused_attention_gpu import edge_pattern, rand, same
from test_torch_attention_gpu import make_A, pattern
from test_torch_autograd_gpu import _close

pytestmark = pytest.mark.gpu

LR = 0.05
INVALID = 9


def grid(rs, rows, H, d, half):
    """(rows, H, d) fp32 on the grid: i / 32 (half = False) or (i + 1/2) / 32 (half = True), i uniform in [-32, 32]"""
    i = rs.randint(-32, 33, size=(rows, H, d)).astype(np.float64)
    return ((i + (0.5 if half else 0.0)) / 32.0).astype(np.float32)


def assert_off_the_kink(rp, ci, xdn, xsn):
    """float64 z = x_dst[r, h, k] + x_src[c, h, k] of every stored entry, head and k stays away from LeakyReLU's kink"""
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    z = xdn.astype(np.float64)[rows] + xsn.astype(np.float64)[ci]
    assert z.size == 0 or np.all(np.abs(z) > 1e-5), float(np.abs(z).min())


def reference(rp, ci, M, K, xdn, xsn, attn, Gn, slope, bias_values=None, shared=False):
    """float64 on the edge list with torch autograd: O (M, H, d), dxd, dxs (shared: dx, their sum, under both names), datt_rows
    (M, H, d) -- att enters as one copy per row, whose gradient is the row's share --, datt, and the bias gradient dA (nnz) or None"""
    import torch
    H, d = xdn.shape[1], xdn.shape[2]
    rows = torch.from_numpy(np.repeat(np.arange(M), np.diff(rp)).astype(np.int64))
    cols = torch.from_numpy(ci.astype(np.int64))
    xd = torch.from_numpy(xdn).double().requires_grad_()
    xs = xd if shared else torch.from_numpy(xsn).double().requires_grad_()
    at_rows = torch.from_numpy(attn).double()[None].repeat(M, 1, 1).requires_grad_()
    b = torch.from_numpy(bias_values).double().requires_grad_() if bias_values is not None else None
    z = xd[rows] + xs[cols]                                                         # (nnz, H, d)
    s = (torch.nn.functional.leaky_relu(z, slope) * at_rows[rows]).sum(-1)          # (nnz, H)
    if b is not None:
        s = s + b[:, None]
    idx = rows[:, None].expand(-1, H)
    m = torch.full((M, H), float("-inf"), dtype=torch.float64).scatter_reduce(0, idx, s.detach(), "amax", include_self=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m[rows])
    Z = torch.zeros((M, H), dtype=torch.float64).index_add(0, rows, e)
    p = e / Z[rows]
    O = torch.zeros((M, H, d), dtype=torch.float64).index_add(0, rows, p[:, :, None] * xs[cols])
    O.backward(torch.from_numpy(Gn).double())
    n = lambda t: t.detach().numpy()   # noqa: E731
    return {"O": n(O), "dxd": n(xd.grad), "dxs": n(xs.grad), "datt_rows": n(at_rows.grad), "datt": n(at_rows.grad.sum(0)),
            "dA": n(b.grad) if b is not None else None}


def run(rp, ci, v, M, K, xdn, xsn, attn, Gn, slope, bias, squeeze=False):
    """-> (O, dx_dst, dx_src, datt, dA values or None) as numpy, heads on axis 1; squeeze: hand H = 1 operands over as 2-D (att: 1-D)"""
    import torch
    from sextans_amd import torch_op
    A = make_A(rp, ci, v, M, K, grad=bias)
    xd, xs = (torch.from_numpy(t[:, 0] if squeeze else t).cuda().requires_grad_() for t in (xdn, xsn))
    at = torch.from_numpy(attn[0] if squeeze else attn).cuda().requires_grad_()
    out = torch_op.gatv2_attention(A, xd, xs, at, negative_slope=slope, bias=bias)
    assert out.dim() == xd.dim()
    out.backward(torch.from_numpy(Gn[:, 0] if squeeze else Gn).cuda())
    if bias:
        assert A.grad.layout == torch.sparse_csr and A.grad.values().dtype == A.values().dtype
    else:
        assert A.grad is None
    assert xd.grad.shape == xd.shape and xs.grad.shape == xs.shape and at.grad.shape == at.shape and at.grad.dtype == at.dtype
    res = [t.detach().cpu().numpy() for t in (out, xd.grad, xs.grad)]
    if squeeze:
        res = [t[:, None] for t in res]
    datt = at.grad.cpu().numpy()
    return res + [datt[None] if squeeze else datt, A.grad.values().cpu().numpy() if bias else None]


def check(got, want, bias):
    for g, k in zip(got, ("O", "dxd", "dxs", "datt")):
        assert g.shape == want[k].shape, k
        assert np.all(np.isfinite(g)), k
        assert _close(g, want[k]), (k, float(np.abs(g - want[k]).max()))
    if bias:
        assert _close(got[4], want["dA"]), ("dA", float(np.abs(got[4] - want["dA"]).max()))


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("H, d, slope", [(1, 16, 0.2), (3, 24, 0.2), (2, 64, 0.2), (2, 40, 0.2), (1, 128, 0.2), (3, 8, 0.0)])
def test_against_float64_on_the_edge_list(sx, H, d, slope, bias):
    from sextans_amd import torch_op
    M, K = 300, 260
    rs, rp, ci, v = pattern(31 + d, M, K, 9)
    assert np.all(np.diff(rp) > 0)
    xdn, xsn, attn, Gn = grid(rs, M, H, d, False), grid(rs, K, H, d, True), rand(rs, H, d), rand(rs, M, H, d)
    assert_off_the_kink(rp, ci, xdn, xsn)
    torch_op.clear_cache()
    got = run(rp, ci, v, M, K, xdn, xsn, attn, Gn, slope, bias, squeeze=(H == 1 and d == 16))
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0, info
    want = reference(rp, ci, M, K, xdn, xsn, attn, Gn, slope, v if bias else None)
    check(got, want, bias)
    torch_op.clear_cache()


def test_row_length_edges_and_long_rows(sx):
    import torch
    from sextans_amd import torch_op
    rs = np.random.RandomState(8)
    rp, ci, v, M, K = edge_pattern(rs)
    assert M < 3000 and np.count_nonzero(ci == 0) > 2048 and np.diff(rp).max() == 2500
    H, d = 2, 16
    xdn, xsn, attn, Gn = grid(rs, M, H, d, False), grid(rs, K, H, d, True), rand(rs, H, d), rand(rs, M, H, d)
    assert_off_the_kink(rp, ci, xdn, xsn)
    torch_op.clear_cache()
    got = run(rp, ci, v, M, K, xdn, xsn, attn, Gn, 0.2, True)
    eng = next(iter(torch_op._cache.values())).eng
    assert eng.last_kernel() == "gatv2_fused_backward+long_rows"
    want = reference(rp, ci, M, K, xdn, xsn, attn, Gn, 0.2, v)
    check(got, want, True)
    ones = np.flatnonzero(np.diff(rp) == 1)   # a row of one entry: p = 1, O is x_src's row
    assert len(ones) == 2101
    assert same(got[0][ones], xsn[ci[rp[ones]]])
    # the forward alone names its own kernel
    A = make_A(rp, ci, v, M, K)
    torch_op.gatv2_attention(A, *(torch.from_numpy(t).cuda() for t in (xdn, xsn, attn)))
    assert list(torch_op._cache.values())[-1].eng.last_kernel() == "gatv2_fused+long_rows"   # (A's new index tensors: a new entry)
    torch_op.clear_cache()


class Abi:
    """one engine on a pattern, operands as torch tensors, the entry points called through api.Engine"""

    def __init__(self, sx, rp, ci, M, K, H, d):
        import torch
        self.t = torch
        self.M, self.K, self.H, self.d, self.nnz = M, K, H, d, len(ci)
        self.rp, self.ci = torch.from_numpy(rp.astype(np.int32)).cuda(), torch.from_numpy(ci.astype(np.int32)).cuda()
        self.ci_arg = self.ci if len(ci) else torch.zeros(1, dtype=torch.int32, device="cuda")
        self.val = torch.full((max(len(ci), 1),), float("nan"), device="cuda")   # A's own values are not read
        self.eng = sx.Engine(0)
        self.eng.set_matrix_csr_device(M, K, len(ci), self.rp.data_ptr(), self.ci_arg.data_ptr(), self.val.data_ptr())

    def forward(self, xd, xs, att, bias, slope):
        t, H, d = self.t, self.H, self.d
        O = t.full((max(self.M, 1), H, d), 7.0, device="cuda"); lse = t.full((max(self.M, 1), H), 7.0, device="cuda")
        self.eng.gatv2_attention_device(H, d, slope, xd.data_ptr(), H * d, xs.data_ptr(), H * d, att.data_ptr(),
                                        bias.data_ptr() if bias is not None else None, O.data_ptr(), H * d, lse.data_ptr(),
                                        t.cuda.current_stream().cuda_stream)
        return O[:self.M], lse[:self.M]

    def gat_forward(self, ad, as_, V, slope):
        t, H, d = self.t, self.H, self.d
        O = t.full((self.M, H, d), 7.0, device="cuda"); lse = t.full((self.M, H), 7.0, device="cuda")
        self.eng.gat_attention_device(H, d, slope, ad.data_ptr(), H, as_.data_ptr(), H, V.data_ptr(), H * d, None, O.data_ptr(), H * d,
                                      lse.data_ptr(), t.cuda.current_stream().cuda_stream)
        return O, lse

    def backward(self, xd, xs, att, bias, slope, O, lse, G, want_dbias=True):
        """-> dx_dst, dx_src, datt, dbias; self.delta, self.work (datt_rows, then part) keep the workspaces"""
        t, H, d = self.t, self.H, self.d
        full = lambda *s: t.full(tuple(max(x, 1) for x in s), 7.0, device="cuda")   # noqa: E731  (never a NULL pointer of its own accord)
        delta, dxd, dxs, datt = full(self.M, H), full(self.M, H, d), full(self.K, H, d), full(H, d)
        nwork = self.eng.gatv2_workspace_floats(H, d)
        assert nwork == self.M * H * d + -(-self.M // 256) * H * d
        work = full(nwork + 8)
        db = full(self.nnz) if want_dbias else None
        self.eng.gatv2_attention_backward_device(H, d, slope, xd.data_ptr(), H * d, xs.data_ptr(), H * d, att.data_ptr(),
                                                 bias.data_ptr() if bias is not None else None, O.data_ptr(), H * d, lse.data_ptr(), G.data_ptr(),
                                                 H * d, delta.data_ptr(), dxd.data_ptr(), H * d, dxs.data_ptr(), H * d, datt.data_ptr(),
                                                 work.data_ptr(), db.data_ptr() if db is not None else None, t.cuda.current_stream().cuda_stream)
        assert bool((work[nwork:] == 7.0).all())   # nothing is written past the size the query gave
        self.delta, self.work = delta[:self.M], work[:nwork]
        return dxd[:self.M], dxs[:self.K], datt, (db[:self.nnz] if db is not None else None)


@pytest.mark.parametrize("d", [8, 24, 64, 128])
def test_forward_has_the_bits_of_the_gat_kernel(sx, d):
    """att[h, :] = (1, 0, .., 0), no bias: the score is leaky_relu(x_dst[r, h, 0] + x_src[c, h, 0]) exactly (a fused multiply-add with a
    zero factor and the zeros the slot's butterfly adds change nothing; the grid keeps l[0] away from 0), which is the GAT kernel's
    score for a_dst = x_dst[..., 0], a_src = x_src[..., 0]; with V = x_src both kernels then form the same batches."""
    import torch
    rs = np.random.RandomState(5)
    rp, ci, _, M, K = edge_pattern(rs)
    H = 2
    xdn, xsn = grid(rs, M, H, d, False), grid(rs, K, H, d, True)
    attn = np.zeros((H, d), np.float32); attn[:, 0] = 1.0
    xd, xs, att = (torch.from_numpy(t).cuda() for t in (xdn, xsn, attn))
    ad, as_ = xd[:, :, 0].contiguous(), xs[:, :, 0].contiguous()
    a = Abi(sx, rp, ci, M, K, H, d)
    O, lse = a.forward(xd, xs, att, None, 0.2)
    assert a.eng.last_kernel() == "gatv2_fused+long_rows"
    O2, lse2 = a.gat_forward(ad, as_, xs, 0.2)
    assert a.eng.last_kernel() == "gat_fused+long_rows"
    On, O2n, lsen, lse2n = (x.cpu().numpy() for x in (O, O2, lse, lse2))
    assert np.all(np.isfinite(On)) and np.all(np.isfinite(lsen))
    assert same(On, O2n), int(np.count_nonzero(On.view(np.uint32) != O2n.view(np.uint32)))
    assert same(lsen, lse2n), int(np.count_nonzero(lsen.view(np.uint32) != lse2n.view(np.uint32)))
    a.eng.close()


def test_datt_is_summed_in_the_documented_order(sx):
    """level 1: per chunk of 256 rows, ascending, from +0; level 2: over the chunks, ascending, from +0 -- recomputed add by add"""
    import torch
    rs = np.random.RandomState(12)
    rp, ci, v, M, K = edge_pattern(rs)
    assert M == 2112 and M % 256 != 0 and M > 2 * 256
    H, d = 2, 16
    hd = H * d
    xdn, xsn, attn, Gn = grid(rs, M, H, d, False), grid(rs, K, H, d, True), rand(rs, H, d), rand(rs, M, H, d)
    assert_off_the_kink(rp, ci, xdn, xsn)
    xd, xs, att, G, bias = (torch.from_numpy(t).cuda() for t in (xdn, xsn, attn, Gn, v))
    a = Abi(sx, rp, ci, M, K, H, d)
    O, lse = a.forward(xd, xs, att, bias, 0.2)
    datt = a.backward(xd, xs, att, bias, 0.2, O, lse, G)[2].cpu().numpy().reshape(hd)
    assert a.eng.last_kernel() == "gatv2_fused_backward+long_rows"
    work = a.work.cpu().numpy()
    nchunks = -(-M // 256)
    assert work.size == M * hd + nchunks * hd
    datt_rows, part = work[:M * hd].reshape(M, hd), work[M * hd:].reshape(nchunks, hd)
    want_part = np.zeros((nchunks, hd), np.float32)
    for c in range(nchunks):
        s = np.zeros(hd, np.float32)
        for r in range(256 * c, min(256 * c + 256, M)):
            s = s + datt_rows[r]           # (fp32 element by element, rounded to nearest: one add per row, ascending)
        want_part[c] = s
    want = np.zeros(hd, np.float32)
    for c in range(nchunks):
        want = want + want_part[c]
    assert want.dtype == np.float32 and same(part, want_part) and same(datt, want)
    ref = reference(rp, ci, M, K, xdn, xsn, attn, Gn, 0.2, v)
    assert _close(datt_rows.reshape(M, H, d), ref["datt_rows"]), float(np.abs(datt_rows.reshape(M, H, d) - ref["datt_rows"]).max())
    assert _close(datt.reshape(H, d), ref["datt"])
    a.eng.close()


def test_determinism_and_captured_training_step(sx):
    """two eager runs and one on a side stream: the same bits in every output, datt included; then forward, backward and an SGD update
    of x_dst, x_src and att in place, captured once and replayed twice: bit for bit the eager steps, on one engine."""
    import torch
    from sextans_amd import torch_op
    M, K, H, d = 900, 900, 2, 16
    rs, rp, ci, v = pattern(21, M, K, 10)
    xdn, xsn, attn, Gn = grid(rs, M, H, d, False), grid(rs, K, H, d, True), rand(rs, H, d), rand(rs, M, H, d)
    G = torch.from_numpy(Gn).cuda()
    torch_op.clear_cache()
    first = run(rp, ci, v, M, K, xdn, xsn, attn, Gn, 0.2, True)
    second = run(rp, ci, v, M, K, xdn, xsn, attn, Gn, 0.2, True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = run(rp, ci, v, M, K, xdn, xsn, attn, Gn, 0.2, True)
    torch.cuda.current_stream().wait_stream(side)
    for other in (second, third):
        for x, y in zip(first, other):
            assert same(x, y)

    def start():
        A = make_A(rp, ci, v, M, K)
        with torch.no_grad():
            A.values().mul_(0.5)          # (in place: moves the version counter of A's index tensors too)
        return A, [torch.from_numpy(t).cuda().requires_grad_() for t in (xdn, xsn, attn)]

    def step(A, params):
        for t in params:
            t.grad = None
        out = torch_op.gatv2_attention(A, *params, bias=True)
        out.backward(G)
        with torch.no_grad():
            for t in params:
                t.sub_(LR * t.grad)
        return out

    def state(out, params):
        return [out.detach().cpu().numpy().copy()] + [t.detach().cpu().numpy().copy() for t in params]

    torch_op.clear_cache()
    A, params = start()
    eager = [state(step(A, params), params) for _ in range(3)]
    assert not np.array_equal(eager[2][3], eager[0][3])
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
    for k in range(1, 3):
        g.replay()
        torch.cuda.synchronize()
        got = state(out, params)
        for i in range(4):
            assert same(got[i], eager[k][i]), (k, i)
    torch_op.clear_cache()


@pytest.mark.parametrize("slope", [0.2, 0.0])
def test_empty_rows_and_masks_on_the_c_abi(sx, slope):
    import torch
    from util import random_csr
    rs = np.random.RandomState(17)
    M, K, H, d = 400, 400, 2, 24
    rp, ci, _ = random_csr(rs, M, K - 20, 6, empty_frac=0.2)   # the last 20 columns have no entry
    lens = np.diff(rp)
    empty = np.flatnonzero(lens == 0)
    assert len(empty) > 20
    nnz = len(ci)
    xdn, xsn, attn, Gn = grid(rs, M, H, d, False), grid(rs, K, H, d, True), rand(rs, H, d), rand(rs, M, H, d)
    assert_off_the_kink(rp, ci, xdn, xsn)
    bias_n = rand(rs, nnz)
    masked = rp[np.flatnonzero(lens >= 2)]   # rows of two or more entries: their first entry is masked out (-inf)
    assert len(masked) > 100
    bias_n[masked] = -np.inf
    xd, xs, att, G = (torch.from_numpy(t).cuda() for t in (xdn, xsn, attn, Gn))
    bias = torch.from_numpy(bias_n).cuda()
    a = Abi(sx, rp, ci, M, K, H, d)
    O, lse = a.forward(xd, xs, att, bias, slope)
    dxd, dxs, datt, db = a.backward(xd, xs, att, bias, slope, O, lse, G)
    assert a.eng.last_kernel() == "gatv2_fused_backward"
    On, lsen, dxdn, dxsn, dattn, dbn = (x.cpu().numpy() for x in (O, lse, dxd, dxs, datt, db))
    rows_n = a.work.cpu().numpy()[:M * H * d].reshape(M, H, d)
    for x in (On, dxdn, dxsn, dattn, dbn, rows_n, a.delta.cpu().numpy()):
        assert not np.any(np.isnan(x))
    # empty rows: O = +0 (the bits), lse = -inf, zero gradient and datt_rows rows; columns without entries: zero dx_src rows
    assert np.all(On[empty].view(np.uint32) == 0) and np.all(lsen[empty] == -np.inf) and np.all(dxdn[empty] == 0) and np.all(rows_n[empty] == 0)
    assert np.all(np.isfinite(lsen[lens > 0])) and np.all(dxsn[K - 20:] == 0)
    # a -inf entry beside finite ones contributes exactly 0: the results of the pattern without those entries
    assert np.all(dbn[masked] == 0)
    keep = np.ones(nnz, bool); keep[masked] = False
    rows = np.repeat(np.arange(M), lens)
    rp2 = np.zeros(M + 1, np.int32); rp2[1:] = np.cumsum(np.bincount(rows[keep], minlength=M))
    b = Abi(sx, rp2, ci[keep], M, K, H, d)
    bias2 = torch.from_numpy(bias_n[keep]).cuda()
    O2, lse2 = b.forward(xd, xs, att, bias2, slope)
    dxd2, dxs2, datt2, db2 = b.backward(xd, xs, att, bias2, slope, O2, lse2, G)
    assert _close(On, O2.cpu().numpy()) and _close(lsen[lens > 0], lse2.cpu().numpy()[lens > 0])
    assert _close(dxdn, dxd2.cpu().numpy()) and _close(dxsn, dxs2.cpu().numpy()) and _close(dattn, datt2.cpu().numpy())
    assert _close(dbn[keep], db2.cpu().numpy())
    # ... and both agree with the float64 reference on the reduced pattern
    want = reference(rp2, ci[keep], M, K, xdn, xsn, attn, Gn, slope, bias_n[keep])
    check([On, dxdn, dxsn, dattn, dbn[keep]], want, True)
    # a NULL operand with nnz > 0 is refused; without bias and dbias the call is complete
    with pytest.raises(sx.api.SextansError) as err:
        a.eng.gatv2_attention_device(H, d, slope, xd.data_ptr(), H * d, None, H * d, att.data_ptr(), None, O.data_ptr(), H * d, lse.data_ptr(), None)
    assert err.value.code == INVALID
    O3, lse3 = a.forward(xd, xs, att, None, slope)
    dxd3 = a.backward(xd, xs, att, None, slope, O3, lse3, G, want_dbias=False)[0]
    assert np.all(np.isfinite(O3.cpu().numpy())) and np.all(np.isfinite(dxd3.cpu().numpy()))
    # no entries at all, and no rows at all: everything is written, nothing is launched on the pattern
    c = Abi(sx, np.zeros(M + 1, np.int32), np.zeros(0, np.int32), M, K, H, d)
    O4, lse4 = c.forward(xd, xs, att, None, slope)
    dxd4, dxs4, datt4, _ = c.backward(xd, xs, att, None, slope, O4, lse4, G, want_dbias=False)
    assert np.all(O4.cpu().numpy().view(np.uint32) == 0) and np.all(lse4.cpu().numpy() == -np.inf)
    assert all(np.all(x.cpu().numpy() == 0) for x in (dxd4, dxs4, datt4, c.delta, c.work))
    z = Abi(sx, np.zeros(1, np.int32), np.zeros(0, np.int32), 0, K, H, d)
    none = torch.zeros((1, H, d), device="cuda")
    O5, lse5 = z.forward(none, xs, att, None, slope)
    dxd5, dxs5, datt5, _ = z.backward(none, xs, att, None, slope, none, none, none, want_dbias=False)
    assert O5.shape[0] == 0 and dxd5.shape[0] == 0 and z.work.numel() == 0
    assert np.all(dxs5.cpu().numpy() == 0) and np.all(datt5.cpu().numpy() == 0)
    for e in (a, b, c, z):
        e.eng.close()


def test_shared_weights(sx):
    """x_dst and x_src the same leaf on a square pattern (GATv2Conv's share_weights=True): its gradient is the sum of both parts.
    (One grid cannot serve both sides -- i + j may be 0 --, so the shared features are (i + 1/4) / 32: z = (i + j + 1/2) / 32 again.)"""
    import torch
    from sextans_amd import torch_op
    M, H, d = 280, 2, 24
    rs, rp, ci, v = pattern(61, M, M, 8)
    xn = ((rs.randint(-32, 33, size=(M, H, d)) + 0.25) / 32.0).astype(np.float32)
    attn, Gn = rand(rs, H, d), rand(rs, M, H, d)
    assert_off_the_kink(rp, ci, xn, xn)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, M, grad=True)
    x, at = torch.from_numpy(xn).cuda().requires_grad_(), torch.from_numpy(attn).cuda().requires_grad_()
    out = torch_op.gatv2_attention(A, x, x, at, bias=True)
    out.backward(torch.from_numpy(Gn).cuda())
    want = reference(rp, ci, M, M, xn, xn, attn, Gn, 0.2, v, shared=True)
    n = lambda t: t.detach().cpu().numpy()   # noqa: E731
    assert _close(n(out), want["O"]) and _close(n(x.grad), want["dxd"]) and _close(n(at.grad), want["datt"])
    assert _close(n(A.grad.values()), want["dA"])
    torch_op.clear_cache()


def test_operand_placement(sx):
    import torch
    from sextans_amd import torch_op
    from sextans_amd.torch_op import _heads_operand
    M, K, H, d = 260, 240, 2, 24
    rs, rp, ci, v = pattern(51, M, K, 8)
    xdn, xsn, attn, Gn = grid(rs, M, H, d, False), grid(rs, K, H, d, True), rand(rs, H, d), rand(rs, M, H, d)
    torch_op.clear_cache()
    base = run(rp, ci, v, M, K, xdn, xsn, attn, Gn, 0.2, False)[:4]

    def outcome(xd, xs):
        A = make_A(rp, ci, v, M, K)
        at = torch.from_numpy(attn).cuda().requires_grad_()
        out = torch_op.gatv2_attention(A, xd, xs, at)
        out.backward(torch.from_numpy(Gn).cuda())
        return [t.detach().cpu().numpy() for t in (out, xd.grad, xs.grad, at.grad)]

    def in_wider_buffer(t, pad, off):
        """(rows, H, w) as columns [off, off + H w) of a (rows, H w + pad) buffer: a leaf the kernels read where it lies"""
        rows, h, w = t.shape
        buf = torch.full((rows, h * w + pad), 9.0, device="cuda")
        view = buf[:, off:off + h * w].unflatten(1, (h, w))
        view.copy_(torch.from_numpy(t))
        assert view.stride(0) > h * w and not view.is_contiguous()
        return view.detach().requires_grad_()

    # column-sliced views with ld > H d, 16-byte aligned: accepted without a copy, the bits of the contiguous operands
    wide = [in_wider_buffer(xdn, 8, 4), in_wider_buffer(xsn, 12, 8)]
    assert all(w.data_ptr() % 16 == 0 and w.stride(0) % 4 == 0 for w in wide)
    assert _heads_operand(wide[0].detach(), d)[0].data_ptr() == wide[0].data_ptr() and _heads_operand(wide[1].detach(), d)[1] == H * d + 12
    for x, y in zip(outcome(*wide), base):
        assert same(x, y)
    # a row stride that is not a multiple of 4: copied, the same bits
    odd = [in_wider_buffer(xdn, 6, 4), in_wider_buffer(xsn, 5, 0)]
    assert all(w.stride(0) % 4 != 0 for w in odd)
    assert all(_heads_operand(w.detach(), d)[0].data_ptr() != w.data_ptr() and _heads_operand(w.detach(), d)[1] == H * d for w in odd)
    for x, y in zip(outcome(*odd), base):
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
        torch_op.gatv2_attention(A, z(M, 3, 16), z(K, 2, 16), z(2, 16))        # heads
    with pytest.raises(ValueError):
        torch_op.gatv2_attention(A, z(M, 2, 16), z(K, 2, 16), z(3, 16))
    with pytest.raises(ValueError):
        torch_op.gatv2_attention(A, z(M, 2, 16), z(K, 2, 16), z(16))           # ranks
    with pytest.raises(ValueError):
        torch_op.gatv2_attention(A, z(M, 16), z(K, 1, 16), z(16))
    with pytest.raises(ValueError):
        torch_op.gatv2_attention(A, z(M - 1, 2, 16), z(K, 2, 16), z(2, 16))    # rows
    with pytest.raises(ValueError):
        torch_op.gatv2_attention(A, z(M, 2, 16), z(M, 2, 16), z(2, 16))
    with pytest.raises(ValueError):
        torch_op.gatv2_attention(A, z(M, 2, 16), z(K, 2, 24), z(2, 16))        # d
    with pytest.raises(ValueError):
        torch_op.gatv2_attention(A, z(M, 136), z(K, 136), z(136))
    with pytest.raises(ValueError):
        torch_op.gatv2_attention(A, z(M, 16), z(K, 16), z(16), negative_slope=-0.1)
    with pytest.raises(TypeError):
        torch_op.gatv2_attention(A, z(M, 2, 16).cpu(), z(K, 2, 16), z(2, 16))
    with pytest.raises(TypeError):
        torch_op.gatv2_attention(A.cpu(), z(M, 2, 16), z(K, 2, 16), z(2, 16))
    torch_op.clear_cache()
