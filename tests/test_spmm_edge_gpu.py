"""SpMM with a feature vector per entry on the GPU (sextans_spmm_edge_device_rm, sextans_spmm_edge_backward_device_rm,
torch_op.spmm_edge, torch_op.from_edge_index): exact on integer operands for every tile width, op and lane-group size; random floats
within the worst-case bound of fp32 summation in ANY order, |got - want| <= (len + 1) 2^-23 sum |term| (gamma_len plus the terms' own
rounding; want and the magnitudes in float64), with operands read and written where they lie; dE bit for bit the numpy float32
expression; empty rows, unused columns, NaN / inf, degenerate matrices, autograd, reproducibility and graph capture."""
import numpy as np
import pytest

from test_fused_attention_gpu import edge_pattern, rand
from test_torch_attention_gpu import make_A, pattern
from util import random_csr

pytestmark = pytest.mark.gpu

OPS = {"mul": 1, "add": 2, "add_relu": 3, "copy": 4}
EPS = 2.0 ** -23


def rows_of(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


def messages(op, Bc, E):
    """the messages of all entries from the gathered B rows, in the operands' dtype (float32: one rounded operation each)"""
    if op == "mul":
        return Bc * E
    if op == "add":
        return Bc + E
    if op == "add_relu":
        s = Bc + E
        return np.where(s > 0, s, np.where(np.isnan(s), s, np.zeros_like(s)))
    return E.copy()


def scatter(idx, terms, n):
    out = np.zeros((n,) + terms.shape[1:], terms.dtype)
    np.add.at(out, idx, terms)
    return out


def reference(op, rp, ci, B, E, G, K, dtype=np.float64):
    """C, dB (None for copy), dE and the sums of the terms' magnitudes behind C and dB, all computed in `dtype`"""
    M = len(rp) - 1
    rows = rows_of(rp)
    Bc = B.astype(dtype)[ci] if op != "copy" else None
    E, Gr = E.astype(dtype), G.astype(dtype)[rows]
    m = messages(op, Bc, E)
    C, absC = scatter(rows, m, M), scatter(rows, np.abs(m), M)
    zero = np.zeros_like(Gr)
    if op == "mul":
        dE, tB = Gr * Bc, Gr * E
    elif op == "add_relu":
        dE = np.where(Bc + E > 0, Gr, zero)
        tB = dE
    else:
        dE, tB = Gr.copy(), Gr
    if op == "copy":
        return C, None, dE, absC, None
    return C, scatter(ci, tB, K), dE, absC, scatter(ci, np.abs(tB), K)


def bits_equal(got, want):
    return got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def within_bound(got, want, mags, lens, what=""):
    """the worst case of an fp32 sum of len terms in any order, the terms themselves rounded once"""
    bound = (lens[:, None] + 1) * EPS * mags
    err = np.abs(got.astype(np.float64) - want)
    print(what, "max |got - want|", float(err.max()) if err.size else 0.0, "max err / bound",
          float((err[bound > 0] / bound[bound > 0]).max()) if np.any(bound > 0) else 0.0)
    return bool(np.all(err <= bound))


class Abi:
    """one engine on a pattern, operands as torch tensors, the two entry points called through api.Engine"""

    def __init__(self, sx, rp, ci, M, K):
        import torch
        self.t = torch
        self.M, self.K, self.nnz = M, K, len(ci)
        self.rp, self.ci = torch.from_numpy(rp.astype(np.int32)).cuda(), torch.from_numpy(ci.astype(np.int32)).cuda()
        self.val = torch.ones(max(self.nnz, 4), device="cuda")
        self.eng = sx.Engine(0)
        self.eng.set_matrix_csr_device(M, K, self.nnz, self.rp.data_ptr(), self.ci.data_ptr(), self.val.data_ptr())

    def buf(self, a, pad, fill=float("nan")):
        """a (rows, N) numpy -> a (rows, N + pad) device buffer whose padding columns hold `fill`"""
        out = self.t.full((max(a.shape[0], 1), a.shape[1] + pad), fill, device="cuda")
        out[:a.shape[0], :a.shape[1]] = self.t.from_numpy(a)
        return out

    def forward(self, op, B, E, pad=(0, 0, 0)):
        """-> C as numpy and the whole C buffer; pad: extra columns of the B / E / C buffers"""
        t = self.t
        N = E.shape[1]
        Bb = self.buf(B, pad[0]) if op != "copy" else None
        Eb = self.buf(E, pad[1])
        Cb = t.full((max(self.M, 1), N + pad[2]), 7.0, device="cuda")
        self.eng.spmm_edge_device_rm(OPS[op], N, Bb.data_ptr() if Bb is not None else None, N + pad[0], Eb.data_ptr(), N + pad[1],
                                     Cb.data_ptr(), N + pad[2], t.cuda.current_stream().cuda_stream)
        t.cuda.synchronize()
        Cn = Cb.cpu().numpy()[:self.M]
        return Cn[:, :N], Cn

    def backward(self, op, B, E, G, want_dB=True, want_dE=True, pad=(0, 0, 0, 0, 0)):
        """-> dB, dE as numpy (None where not asked for, and dB for copy) and their whole buffers; pad: B / E / G / dB / dE"""
        t = self.t
        N = G.shape[1]
        want_dB = want_dB and op != "copy"
        need_b = op == "add_relu" or (op == "mul" and want_dE)
        need_e = op == "add_relu" or (op == "mul" and want_dB)
        Bb = self.buf(B, pad[0]) if need_b else None       # what the op's gradients do not read is passed as NULL
        Eb = self.buf(E, pad[1]) if need_e else None
        Gb = self.buf(G, pad[2])
        dB = t.full((self.K, N + pad[3]), 7.0, device="cuda") if want_dB else None
        dE = t.full((max(self.nnz, 1), N + pad[4]), 7.0, device="cuda") if want_dE else None
        ptr = lambda x: x.data_ptr() if x is not None else None   # noqa: E731
        self.eng.spmm_edge_backward_device_rm(OPS[op], N, ptr(Bb), N + pad[0], ptr(Eb), N + pad[1], Gb.data_ptr(), N + pad[2], ptr(dB),
                                              N + pad[3], ptr(dE), N + pad[4], t.cuda.current_stream().cuda_stream)
        t.cuda.synchronize()
        dBn = dB.cpu().numpy() if want_dB else None
        dEn = dE.cpu().numpy()[:self.nnz] if want_dE else None
        return (dBn[:, :N] if want_dB else None), (dEn[:, :N] if want_dE else None), dBn, dEn


def ints(rs, *shape):
    return rs.randint(-4, 5, size=shape).astype(np.float32)


@pytest.mark.parametrize("N", [8, 16, 24, 64, 136])
def test_exact_on_integers_every_width_and_lane_group(sx, N):
    """all five tile widths, a partial tile (24) and a second, partial tile (136); rows of 1 .. 300 entries around every lane-group size,
    a long row and a long column.  Integer operands in [-4, 4]: every message, product and partial sum is an integer below 2^24, so
    every summation order is exact and C, dB, dE equal the int64 computation."""
    rs = np.random.RandomState(8)
    rp, ci, _, M, K = edge_pattern(rs)
    assert M < 3000 and np.count_nonzero(ci == 0) > 2048 and np.diff(rp).max() == 2500
    B, E, G = ints(rs, K, N), ints(rs, len(ci), N), ints(rs, M, N)
    assert np.any(B[ci] + E == 0)   # the kink of ADD_RELU: its gradient there is 0
    a = Abi(sx, rp, ci, M, K)
    for op in OPS:
        wC, wdB, wdE, _, _ = reference(op, rp, ci, B, E, G, K, dtype=np.int64)
        C, _ = a.forward(op, B, E)
        assert a.eng.last_kernel() == "spmm_edge+long_rows"
        assert np.array_equal(C, wC.astype(np.float32)), op
        dB, dE, _, _ = a.backward(op, B, E, G)
        assert a.eng.last_kernel() == "spmm_edge_backward+long_rows"
        assert np.array_equal(dE, wdE.astype(np.float32)), op
        if op == "copy":
            assert dB is None
            continue
        assert np.array_equal(dB, wdB.astype(np.float32)), op
        if op == "add_relu":
            assert np.all(dE[B[ci] + E == 0] == 0)
        # either gradient alone: the same result
        assert np.array_equal(a.backward(op, B, E, G, want_dE=False)[0], dB) and np.array_equal(a.backward(op, B, E, G, want_dB=False)[1], dE)
    a.eng.close()


@pytest.mark.parametrize("N", [16, 40, 128])
def test_random_floats_operands_where_they_lie(sx, N):
    """every leading dimension N + 4 or N + 8, NaN in the padding of the inputs, 7.0 left alone in the padding of the outputs"""
    M, K = 300, 260
    rs, rp, ci, _ = pattern(31 + N, M, K, 9)
    nnz = len(ci)
    lens, clens = np.diff(rp), np.bincount(ci, minlength=K)
    rows = rows_of(rp)
    B, E, G = rand(rs, K, N), rand(rs, nnz, N), rand(rs, M, N)
    a = Abi(sx, rp, ci, M, K)
    for op in OPS:
        wC, wdB, _, absC, absB = reference(op, rp, ci, B, E, G, K)
        C, Cb = a.forward(op, B, E, pad=(4, 8, 4))
        assert a.eng.last_kernel() == "spmm_edge"
        assert np.all(Cb[:, N:] == 7.0)
        assert within_bound(C, wC, absC, lens, "%s N=%d C" % (op, N)), op
        m32 = messages(op, B[ci] if op != "copy" else None, E)
        one = lens == 1
        assert np.array_equal(C[one], m32[np.isin(rows, np.flatnonzero(one))])   # a row of one entry: the message itself
        dB, dE, dBb, dEb = a.backward(op, B, E, G, pad=(8, 4, 8, 4, 8))
        assert a.eng.last_kernel() == "spmm_edge_backward"
        assert np.all(dEb[:, N:] == 7.0)
        # one rounded float32 operation per element: the bits of the numpy float32 expression
        assert bits_equal(dE, reference(op, rp, ci, B, E, G, K, dtype=np.float32)[2]), op
        if op != "copy":
            assert np.all(dBb[:, N:] == 7.0)
            assert within_bound(dB, wdB, absB, clens, "%s N=%d dB" % (op, N)), op
    a.eng.close()


def test_empty_rows_and_unused_columns(sx):
    rs = np.random.RandomState(17)
    M, K, N = 400, 400, 24
    rp, ci, _ = random_csr(rs, M, 380, 6, empty_frac=0.2)   # the last 20 columns hold no entry
    lens, clens = np.diff(rp), np.bincount(ci, minlength=K)
    assert np.count_nonzero(lens == 0) > 40 and ci.max() < 380
    B, E, G = rand(rs, K, N), rand(rs, len(ci), N), rand(rs, M, N)
    B[380:] = np.nan
    a = Abi(sx, rp, ci, M, K)
    for op in OPS:
        wC, wdB, wdE, absC, absB = reference(op, rp, ci, B, E, G, K)
        C, _ = a.forward(op, B, E)
        assert np.all(np.isfinite(C)) and np.all(C[lens == 0].view(np.uint32) == 0), op
        assert within_bound(C, wC, absC, lens, op + " C")
        dB, dE, _, _ = a.backward(op, B, E, G)
        assert np.all(np.isfinite(dE)) and bits_equal(dE, reference(op, rp, ci, B, E, G, K, dtype=np.float32)[2]), op
        if op != "copy":
            assert np.all(dB[clens == 0] == 0) and np.all(dB[380:] == 0), op
            assert within_bound(dB, wdB, absB, clens, op + " dB")
    a.eng.close()


@pytest.mark.parametrize("op", ["mul", "add"])
def test_special_values(sx, op):
    """a NaN row and a +inf row in B and in E: C is not finite exactly on the rows that own such an entry, dB only on the columns the
    special E entries sit in (MUL; ADD's dB does not read E), dE only where the formula reads them"""
    rs = np.random.RandomState(23)
    M, K, N = 400, 300, 16
    rp, ci, _ = random_csr(rs, M, K, 7, empty_frac=0.1)
    lens, clens, rows = np.diff(rp), np.bincount(ci, minlength=K), rows_of(rp)
    B, E, G = rand(rs, K, N), rand(rs, len(ci), N), rand(rs, M, N)
    cols = np.flatnonzero(clens > 0)
    cn, cinf = cols[3], cols[40]
    en, einf = 11, len(ci) // 2
    B[cn], B[cinf], E[en], E[einf] = np.nan, np.inf, np.nan, np.inf
    special = np.isin(ci, [cn, cinf])
    special[[en, einf]] = True
    owners = np.unique(rows[special])
    assert 2 < len(owners) < M // 2
    a = Abi(sx, rp, ci, M, K)
    with np.errstate(invalid="ignore"):
        wC, wdB, _, absC, absB = reference(op, rp, ci, B, E, G, K)
        wdE = reference(op, rp, ci, B, E, G, K, dtype=np.float32)[2]
    C, _ = a.forward(op, B, E)
    bad = ~np.isfinite(C)
    assert np.array_equal(np.flatnonzero(bad.any(axis=1)), owners) and np.all(bad[owners])
    assert np.array_equal(np.isnan(C), np.isnan(wC)) and np.array_equal(C[np.isinf(C)], wC[np.isinf(wC)].astype(np.float32))
    ok = np.setdiff1d(np.arange(M), owners)
    assert within_bound(C[ok], wC[ok], absC[ok], lens[ok], op + " C")
    dB, dE, _, _ = a.backward(op, B, E, G)
    assert np.array_equal(dE, wdE, equal_nan=True)
    hit = np.unique(ci[[en, einf]]) if op == "mul" else np.zeros(0, np.int64)
    badB = ~np.isfinite(dB)
    assert np.array_equal(np.flatnonzero(badB.any(axis=1)), hit)
    assert np.array_equal(np.isnan(dB), np.isnan(wdB))
    okc = np.setdiff1d(np.arange(K), hit)
    assert within_bound(dB[okc], wdB[okc], absB[okc], clens[okc], op + " dB")
    a.eng.close()


def test_degenerate_matrices(sx):
    rs = np.random.RandomState(3)
    M, K, N = 5, 6, 16
    B, G = rand(rs, K, N), rand(rs, M, N)
    none = np.zeros((0, N), np.float32)
    # no entry at all: C and dB are zero-filled, dE has no element
    a = Abi(sx, np.zeros(M + 1, np.int32), np.zeros(0, np.int32), M, K)
    for op in OPS:
        C, Cb = a.forward(op, B, none, pad=(0, 0, 4))
        assert np.all(C.view(np.uint32) == 0) and np.all(Cb[:, N:] == 7.0), op
        dB, dE, dBb, dEb = a.backward(op, B, none, G, pad=(0, 0, 0, 4, 0))
        assert dE.shape[0] == 0 and np.all(dEb == 7.0)
        if op != "copy":
            assert np.all(dB == 0) and np.all(dBb[:, N:] == 7.0), op
    a.eng.close()
    # no row at all
    z = Abi(sx, np.zeros(1, np.int32), np.zeros(0, np.int32), 0, K)
    for op in OPS:
        C, Cb = z.forward(op, B, none)
        assert C.shape[0] == 0
        dB, dE, _, _ = z.backward(op, B, none, np.zeros((0, N), np.float32))
        assert dE.shape[0] == 0 and (op == "copy" or np.all(dB == 0)), op
    z.eng.close()


def torch_reference(op, reduce, rp, ci, Bn, En, Gn, M):
    """the float64 torch composition on the CPU (gather, op, index_add_) and its autograd -> out, dB (None for copy), dE"""
    import torch
    rows, col = torch.from_numpy(rows_of(rp)).long(), torch.from_numpy(ci).long()
    E = torch.from_numpy(En).double().requires_grad_()
    B = torch.from_numpy(Bn).double().requires_grad_() if op != "copy" else None
    m = {"mul": lambda: B[col] * E, "add": lambda: B[col] + E, "add_relu": lambda: torch.relu(B[col] + E), "copy": lambda: E * 1.0}[op]()
    out = torch.zeros((M,) + tuple(En.shape[1:]), dtype=torch.float64).index_add_(0, rows, m)
    if reduce == "mean":
        deg = torch.from_numpy(np.maximum(np.diff(rp), 1)).double()
        out = out / deg.reshape((M,) + (1,) * (out.dim() - 1))
    out.backward(torch.from_numpy(Gn).double())
    return out.detach().numpy(), (B.grad.numpy() if B is not None else None), E.grad.numpy()


@pytest.mark.parametrize("shape", [(24,), (3, 8)])
@pytest.mark.parametrize("op,reduce", [("mul", "sum"), ("add", "sum"), ("add_relu", "sum"), ("copy", "sum"), ("mul", "mean"), ("add_relu", "mean")])
def test_torch_autograd(sx, op, reduce, shape):
    import torch
    from sextans_amd import torch_op
    M, K = 300, 260
    rs, rp, ci, v = pattern(41, M, K, 9)
    nnz, N = len(ci), int(np.prod(shape))
    lens, clens = np.diff(rp), np.bincount(ci, minlength=K)
    Bn, En, Gn = rand(rs, K, *shape), rand(rs, nnz, *shape), rand(rs, M, *shape)
    if op == "add_relu":   # off the kink, where the derivative is a convention: entries that come close are moved away
        flat = En.reshape(nnz, N)
        flat[np.abs(Bn.reshape(K, N)[ci] + flat) < 1e-3] += np.float32(0.0625)
        assert np.abs(Bn.astype(np.float64)[ci] + En.astype(np.float64)).min() > 1e-5
    wout, wdB, wdE = torch_reference(op, reduce, rp, ci, Bn, En, Gn, M)
    # the bound of the sums, from the float64 magnitudes of their terms; mean: a division on top (one more rounding, in the + 1 ... + 2)
    deg = np.maximum(lens, 1).astype(np.float64)[:, None] if reduce == "mean" else np.ones((M, 1))
    _, _, _, absC, absB = reference(op, rp, ci, Bn.reshape(K, N), En.reshape(nnz, N), Gn.reshape(M, N) / deg, K)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K, grad=True)
    B = torch.from_numpy(Bn).cuda().requires_grad_() if op != "copy" else None
    E = torch.from_numpy(En).cuda().requires_grad_()
    out = torch_op.spmm_edge(A, B, E, op=op, reduce=reduce)
    assert out.shape == (M,) + shape and out.dtype == torch.float32
    out.backward(torch.from_numpy(Gn).cuda())
    n = lambda t: t.detach().cpu().numpy()   # noqa: E731
    extra = 1 if reduce == "mean" else 0
    assert within_bound(n(out).reshape(M, N), wout.reshape(M, N), absC / deg, lens + extra, "%s/%s out" % (op, reduce))
    assert E.grad.shape == E.shape and E.grad.dtype == torch.float32
    # dE: one rounded operation on float32 operands (mean: two, the upstream gradient divided first) against float64
    dE_err = np.abs(n(E.grad).astype(np.float64) - wdE)
    assert np.all(dE_err <= (1 + extra) * EPS * np.abs(wdE))
    if B is not None:
        assert B.grad.shape == B.shape and B.grad.dtype == torch.float32
        assert within_bound(n(B.grad).reshape(K, N), wdB.reshape(K, N), absB, clens + extra, "%s/%s dB" % (op, reduce))
    assert A.grad is None
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0
    # only the gradient that is asked for
    E2 = torch.from_numpy(En).cuda()
    if B is not None:
        B2 = torch.from_numpy(Bn).cuda().requires_grad_()
        torch_op.spmm_edge(A, B2, E2, op=op, reduce=reduce).backward(torch.from_numpy(Gn).cuda())
        assert np.array_equal(n(B2.grad).view(np.uint32), n(B.grad).view(np.uint32))
        assert not torch_op.spmm_edge(A, B2.detach(), E2, op=op).requires_grad
    assert torch_op.cache_info()["engines_built"] == 1
    torch_op.clear_cache()


def test_from_edge_index_and_errors(sx):
    import torch
    from sextans_amd import torch_op
    rs = np.random.RandomState(5)
    num_dst, num_src, N = 90, 70, 16
    cells = rs.choice(num_dst * num_src, size=600, replace=False)   # distinct (dst, src) pairs, in no order
    dst, src = cells // num_src, cells % num_src
    attr, Bn = rand(rs, 600, N), rand(rs, num_src, N)
    want = np.zeros((num_dst, N))
    mags = np.zeros((num_dst, N))
    for i in range(600):   # the per-edge loop over the ORIGINAL list
        t = Bn[src[i]].astype(np.float64) * attr[i].astype(np.float64)
        want[dst[i]] += t
        mags[dst[i]] += np.abs(t)
    edge_index = torch.from_numpy(np.stack([src, dst])).cuda()
    torch_op.clear_cache()
    A, perm = torch_op.from_edge_index(edge_index, num_dst, num_src)
    assert A.layout == torch.sparse_csr and tuple(A.shape) == (num_dst, num_src) and perm.shape == (600,)
    crow, col = A.crow_indices().cpu().numpy(), A.col_indices().cpu().numpy()
    p = perm.cpu().numpy()
    assert np.array_equal(rows_of(crow), dst[p]) and np.array_equal(col, src[p]) and np.all(np.diff(dst[p] * num_src + src[p]) > 0)
    assert np.all(A.values().cpu().numpy() == 1)
    w = torch.from_numpy(rand(rs, 600)).cuda()
    assert torch.equal(torch_op.from_edge_index(edge_index, num_dst, num_src, values=w)[0].values(), w[perm])
    out = torch_op.spmm_edge(A, torch.from_numpy(Bn).cuda(), torch.from_numpy(attr).cuda()[perm])
    assert within_bound(out.cpu().numpy(), want, mags, np.bincount(dst, minlength=num_dst), "from_edge_index")
    doubled = torch.cat([edge_index, edge_index[:, 17:18]], dim=1)
    with pytest.raises(ValueError):
        torch_op.from_edge_index(doubled, num_dst, num_src)
    B, E = torch.from_numpy(Bn).cuda(), torch.from_numpy(attr).cuda()[perm]
    with pytest.raises(ValueError):
        torch_op.spmm_edge(A, B, E, op="max")
    with pytest.raises(ValueError):
        torch_op.spmm_edge(A, B, E, reduce="amax")
    with pytest.raises(ValueError):
        torch_op.spmm_edge(A, None, E)            # B=None only with "copy"
    with pytest.raises(ValueError):
        torch_op.spmm_edge(A, B, E, op="copy")
    with pytest.raises(ValueError):
        torch_op.spmm_edge(A, B, E[:-1])
    with pytest.raises(ValueError):
        torch_op.spmm_edge(A, B[:, :8], E)
    # an N that is no multiple of 8 is padded inside
    out12 = torch_op.spmm_edge(A, B[:, :12], E[:, :12])
    assert out12.shape == (num_dst, 12) and within_bound(out12.cpu().numpy(), want[:, :12], mags[:, :12], np.bincount(dst, minlength=num_dst), "N=12")
    torch_op.clear_cache()


def test_reproducibility_and_capture(sx):
    import torch
    from sextans_amd import torch_op
    rs = np.random.RandomState(8)
    rp, ci, v, M, K = edge_pattern(rs)
    N = 16
    B, E, E2, G = rand(rs, K, N), rand(rs, len(ci), N), rand(rs, len(ci), N), rand(rs, M, N)
    Gt = torch.from_numpy(G).cuda()

    def eager(En):
        A = make_A(rp, ci, v, M, K)
        Bt, Et = torch.from_numpy(B).cuda().requires_grad_(), torch.from_numpy(En).cuda().requires_grad_()
        out = torch_op.spmm_edge(A, Bt, Et, op="mul")
        out.backward(Gt)
        return [t.detach().cpu().numpy() for t in (out, Bt.grad, Et.grad)]

    torch_op.clear_cache()
    first, second = eager(E), eager(E)
    for x, y in zip(first, second):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    one = np.flatnonzero(np.diff(rp) == 1)   # a row of one entry: the message itself
    assert len(one) > 2000 and np.array_equal(first[0][one], B[ci[rp[one]]] * E[rp[one]])
    want = eager(E2)
    assert not np.array_equal(want[0], first[0])

    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    Bt, Et = torch.from_numpy(B).cuda().requires_grad_(), torch.from_numpy(E).cuda().requires_grad_()

    def step():
        Bt.grad = None
        Et.grad = None
        out = torch_op.spmm_edge(A, Bt, Et, op="mul")
        out.backward(Gt)
        return out

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                            # warm-up: engine, softmax tables, A^T and its tables
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    assert torch_op.cache_info()["engines_built"] == 1
    with torch.no_grad():
        Et.copy_(torch.from_numpy(E2).cuda())
    g.replay()
    torch.cuda.synchronize()
    got = [t.detach().cpu().numpy() for t in (out, Bt.grad, Et.grad)]
    for i, (x, y) in enumerate(zip(got, want)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), i
    torch_op.clear_cache()
