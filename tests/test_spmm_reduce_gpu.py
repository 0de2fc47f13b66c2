"""spmm_reduce and the C ABI under it (sextans_spmm_reduce_device_rm, sextans_spmm_reduce_backward_device_rm): max / min aggregation over a
row's entries with the winning entry recorded.  C and arg are bit-determined -- every product is rounded on its own, NaN wins, then the
better product, then the smaller entry -- so the forward is compared EXACTLY (C as uint32, arg as integers) with np.argmax / np.argmin
over each row's fp32 product block, written below, and with torch's CPU torch.sparse.mm(A, B, reduce) -- bit for bit too, but for one
case in which the two references differ from each other on the CPU: where zeros of both signs tie for a row's extreme, torch's kernel
does not keep the sign of the first one (51 and 53 of the 9600 positions of the tie input below); the rule does, and there the result
is compared with torch's as a value.  The gradients are sums: they are
compared with float64 sums built from the reference arg and with torch's CPU autograd under test_torch_autograd_gpu._close (rtol 2e-4,
the tolerance the project holds fp32 sums to).  A comparison of gradients with torch presupposes that no position has a tied extreme
(which entry torch's kernel credits with a tie is its own business): asserted on the CPU first."""
import numpy as np
import pytest

from test_fused_attention_gpu import edge_pattern, rand, same
from test_torch_attention_gpu import make_A
from test_torch_autograd_gpu import _close
from util import random_csr

pytestmark = pytest.mark.gpu

OPS = {"amax": 1, "amin": 2}
POISON = 0x5A5A5A5A


def ref_reduce(rp, ci, v, B, reduce):
    """(C fp32, arg int32) by the rule: per row, np.argmax / np.argmin (NaN wins, the first occurrence wins) over the (entries, N) block
    of fp32 products; an empty row gives +0 and -1"""
    M, N = len(rp) - 1, B.shape[1]
    C, arg = np.zeros((M, N), np.float32), np.full((M, N), -1, np.int32)
    pick = np.argmax if reduce == "amax" else np.argmin
    cols = np.arange(N)
    with np.errstate(all="ignore"):
        for r in range(M):
            b, e = int(rp[r]), int(rp[r + 1])
            if e > b:
                P = v[b:e, None].astype(np.float32) * B[ci[b:e]].astype(np.float32)
                assert P.dtype == np.float32
                k = pick(P, axis=0)
                C[r], arg[r] = P[k, cols], b + k
    return C, arg


def ref_grads(ci, v, B, arg, G, K):
    """float64 dB (K, N) and dval (nnz) from arg: every position's gradient goes to the entry that won it"""
    rows, cols = np.nonzero(arg >= 0)
    e = arg[rows, cols]
    g = G[rows, cols].astype(np.float64)
    dB = np.zeros((K, B.shape[1]))
    np.add.at(dB, (ci[e], cols), v[e].astype(np.float64) * g)
    dval = np.zeros(len(ci))
    np.add.at(dval, e, g * B[ci[e], cols].astype(np.float64))
    return dB, dval


def tied_share(rp, ci, v, B, reduce):
    """share of the (row, column) positions of rows with two or more entries whose extreme is reached by more than one entry"""
    tied = total = 0
    with np.errstate(all="ignore"):
        for r in np.flatnonzero(np.diff(rp) >= 2):
            P = v[rp[r]:rp[r + 1], None] * B[ci[rp[r]:rp[r + 1]]]
            ext = P.max(axis=0) if reduce == "amax" else P.min(axis=0)
            tied += int(np.count_nonzero((P == ext).sum(axis=0) > 1))
            total += P.shape[1]
    return tied / total


def signed_zero_ties(rp, ci, v, B, reduce):
    """(M, N) mask of the positions whose extreme is a zero that the row's products reach with both signs"""
    M, N = len(rp) - 1, B.shape[1]
    mask = np.zeros((M, N), bool)
    for r in np.flatnonzero(np.diff(rp) >= 2):
        P = v[rp[r]:rp[r + 1], None] * B[ci[rp[r]:rp[r + 1]]]
        ext = P.max(axis=0) if reduce == "amax" else P.min(axis=0)
        zero = (P == 0)
        mask[r] = (ext == 0) & np.any(zero & np.signbit(P), axis=0) & np.any(zero & ~np.signbit(P), axis=0)
    return mask


def bits_equal(got, want):
    return got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


class Abi:
    """one engine on a matrix, operands as torch tensors, the two entry points called through api.Engine"""

    def __init__(self, sx, rp, ci, v, M, K):
        import torch
        self.t = torch
        self.M, self.K, self.nnz = M, K, len(ci)
        self.rp, self.ci = torch.from_numpy(rp.astype(np.int32)).cuda(), torch.from_numpy(ci.astype(np.int32)).cuda()
        self.val = torch.zeros(max(self.nnz, 4), device="cuda")
        self.val[:self.nnz] = torch.from_numpy(np.asarray(v, np.float32))
        self.eng = sx.Engine(0)
        self.eng.set_matrix_csr_device(M, K, self.nnz, self.rp.data_ptr(), self.ci.data_ptr(), self.val.data_ptr())

    def forward(self, reduce, B, val=None, want_arg=True, pad=(0, 0, 0), engine_values=False):
        """-> (C, arg) as numpy and the whole padded buffers; B (K, N) numpy; pad: extra columns of the B / C / arg buffers"""
        t = self.t
        N = B.shape[1]
        Bb = t.zeros((self.K, N + pad[0]), device="cuda")
        Bb[:, :N] = t.from_numpy(B)
        Cb = t.full((self.M, N + pad[1]), POISON, dtype=t.int32, device="cuda")
        Ab = t.full((self.M, N + pad[2]), POISON, dtype=t.int32, device="cuda")
        vv = None if engine_values else (self.val if val is None else t.from_numpy(val).cuda())
        self.eng.spmm_reduce_device_rm(OPS[reduce], N, vv.data_ptr() if vv is not None else None, Bb.data_ptr(), N + pad[0], Cb.data_ptr(),
                                       N + pad[1], Ab.data_ptr() if want_arg else None, N + pad[2], t.cuda.current_stream().cuda_stream)
        t.cuda.synchronize()
        Cn, An = Cb.cpu().numpy(), Ab.cpu().numpy()
        return Cn[:, :N].view(np.float32), An[:, :N], Cn, An

    def backward(self, B, arg, G, want_dB=True, want_dval=True, val=None):
        t = self.t
        N = G.shape[1]
        Bt, At, Gt = t.from_numpy(B).cuda(), t.from_numpy(np.ascontiguousarray(arg)).cuda(), t.from_numpy(G).cuda()
        vv = self.val if val is None else t.from_numpy(val).cuda()
        dB = t.full((self.K, N), 7.0, device="cuda") if want_dB else None
        dv = t.full((max(self.nnz, 4),), 7.0, device="cuda") if want_dval else None
        self.eng.spmm_reduce_backward_device_rm(N, vv.data_ptr(), Bt.data_ptr(), N, At.data_ptr(), N, Gt.data_ptr(), N,
                                                dB.data_ptr() if want_dB else None, N, dv.data_ptr() if want_dval else None,
                                                t.cuda.current_stream().cuda_stream)
        t.cuda.synchronize()
        return (dB.cpu().numpy() if want_dB else None), (dv.cpu().numpy()[:self.nnz] if want_dval else None)


def base_matrix(seed):
    rs = np.random.RandomState(seed)
    M, K = 400, 300
    rp, ci, v = random_csr(rs, M, K, 9, empty_frac=0.1, long_rows=1)
    assert np.diff(rp).max() == 300 and np.count_nonzero(np.diff(rp) == 0) > 10
    return rs, rp, ci, v, M, K


@pytest.mark.parametrize("N", [8, 16, 24, 64, 136, 264])
def test_forward_bit_exact_on_the_c_abi(sx, N):
    """one tile, several tiles and a partial last tile; padded leading dimensions with the padding left alone; no arg; the engine's values"""
    import torch
    rs, rp, ci, v, M, K = base_matrix(5)
    B = rand(rs, K, N)
    v2 = rand(rs, len(ci))
    a = Abi(sx, rp, ci, v, M, K)
    for reduce in OPS:
        wantC, wantA = ref_reduce(rp, ci, v, B, reduce)
        C, arg, _, _ = a.forward(reduce, B)
        assert a.eng.last_kernel() == "spmm_reduce"
        assert bits_equal(C, wantC) and np.array_equal(arg, wantA), reduce
        C, arg, Cb, Ab = a.forward(reduce, B, pad=(4, 8, 12))
        assert bits_equal(C, wantC) and np.array_equal(arg, wantA), reduce
        assert np.all(Cb[:, N:] == POISON) and np.all(Ab[:, N:] == POISON)
        C, _, _, Ab = a.forward(reduce, B, want_arg=False)
        assert bits_equal(C, wantC) and np.all(Ab == POISON)
        C, arg, _, _ = a.forward(reduce, B, engine_values=True)
        assert bits_equal(C, wantC) and np.array_equal(arg, wantA), reduce
        # an explicit pointer to other values: the engine's own are not read
        want2 = ref_reduce(rp, ci, v2, B, reduce)
        C, arg, _, _ = a.forward(reduce, B, val=v2)
        assert bits_equal(C, want2[0]) and np.array_equal(arg, want2[1]), reduce
    # new values on the engine: d_val = NULL reads those
    nv = torch.from_numpy(v2).cuda()
    a.eng.update_values_device(nv.data_ptr(), torch.cuda.current_stream().cuda_stream)
    for reduce in OPS:
        want2 = ref_reduce(rp, ci, v2, B, reduce)
        C, arg, _, _ = a.forward(reduce, B, engine_values=True)
        assert bits_equal(C, want2[0]) and np.array_equal(arg, want2[1]), reduce
    a.eng.close()


@pytest.mark.parametrize("N", [16, 40])
def test_row_length_edges_and_long_rows(sx, N):
    rs = np.random.RandomState(8)
    rp, ci, v, M, K = edge_pattern(rs)
    assert M < 3000 and np.count_nonzero(ci == 0) > 2048 and np.diff(rp).max() == 2500
    B, G = rand(rs, K, N), rand(rs, M, N)
    a = Abi(sx, rp, ci, v, M, K)
    for reduce in OPS:
        wantC, wantA = ref_reduce(rp, ci, v, B, reduce)
        C, arg, _, _ = a.forward(reduce, B)
        assert a.eng.last_kernel() == "spmm_reduce+long_rows"
        assert bits_equal(C, wantC) and np.array_equal(arg, wantA), reduce
        wdB, wdv = ref_grads(ci, v, B, wantA, G, K)
        dB, dv = a.backward(B, arg, G)
        assert a.eng.last_kernel() == "spmm_reduce_backward+long_rows"
        print(reduce, N, "max |dB - ref|", float(np.abs(dB - wdB).max()), "max |dval - ref|", float(np.abs(dv - wdv).max()))
        assert _close(dB, wdB) and _close(dv, wdv), reduce
        # either gradient alone: the same bits
        assert same(a.backward(B, arg, G, want_dval=False)[0], dB) and same(a.backward(B, arg, G, want_dB=False)[1], dv)
    a.eng.close()


def tie_inputs():
    rs, rp, ci, _, M, K = base_matrix(12)
    v = rs.choice(np.array([-2, -1, 1, 2], np.float32), len(ci)).astype(np.float32)
    B = rs.randint(-2, 3, (K, 24)).astype(np.float32)
    return rs, rp, ci, v, B, M, K


def test_ties_and_signed_zeros(sx):
    import torch
    rs, rp, ci, v, B, M, K = tie_inputs()
    prod = (v[:, None] * B[ci]).view(np.uint32)
    assert np.any(prod == 0) and np.any(prod == 0x80000000)   # +0 and -0 products
    a = Abi(sx, rp, ci, v, M, K)
    for reduce in OPS:
        share = tied_share(rp, ci, v, B, reduce)
        print(reduce, "tied share", share)
        assert share >= 0.30
        wantC, wantA = ref_reduce(rp, ci, v, B, reduce)
        C, arg, _, _ = a.forward(reduce, B)
        assert bits_equal(C, wantC) and np.array_equal(arg, wantA), reduce
        A_cpu = torch.sparse_csr_tensor(torch.from_numpy(rp.astype(np.int64)), torch.from_numpy(ci.astype(np.int64)), torch.from_numpy(v), size=(M, K))
        # torch's CPU kernel: the same bits, except that among tied zeros of both signs it does not keep the first one's sign -- there the
        # rule above (the first entry wins, as np.argmax has it) and torch differ on the CPU already, in the sign of a zero alone
        tC = torch.sparse.mm(A_cpu, torch.from_numpy(B), reduce).numpy()
        zt = signed_zero_ties(rp, ci, v, B, reduce)
        print(reduce, "positions with zeros of both signs tied for the extreme:", int(zt.sum()), "of", zt.size,
              "; torch's sign differs from the rule's in", int(np.count_nonzero(wantC.view(np.uint32) != tC.view(np.uint32))))
        assert np.array_equal(wantC.view(np.uint32)[~zt], tC.view(np.uint32)[~zt]) and np.all(tC[zt] == 0)
        assert np.array_equal(C.view(np.uint32)[~zt], tC.view(np.uint32)[~zt]) and np.array_equal(C, tC), reduce
    a.eng.close()


def test_infinities_and_nans(sx):
    rs, rp, ci, v, B, M, K = tie_inputs()
    lens = np.diff(rp)
    B = B.copy()
    N = B.shape[1]
    B[rs.randint(0, K, 40), rs.randint(0, N, 40)] = np.inf       # (A's values are non-zero: no 0 * inf)
    B[rs.randint(0, K, 40), rs.randint(0, N, 40)] = -np.inf
    short = int(np.flatnonzero((lens >= 5) & (lens <= 12))[0])
    hub = int(np.argmax(lens))
    assert lens[hub] == 300
    spots = {}                                                    # row -> (first, middle, last entry), its four columns of B
    for r, n0 in ((short, 0), (hub, 4)):
        b, e = int(rp[r]), int(rp[r + 1])
        spots[r] = ((b, b + (e - b) // 2, e - 1), n0)
    nan_cols = {int(ci[e]) for pos, _ in spots.values() for e in pos}
    # a row whose products are all -inf, in every column (it shares no column of A with the NaNs placed below)
    dead = int([r for r in np.flatnonzero(lens == 4) if not nan_cols & set(ci[rp[r]:rp[r + 1]].tolist())][0])
    for e in range(rp[dead], rp[dead + 1]):
        B[ci[e], :] = -np.inf * np.sign(v[e])
    for (first, mid, last), n0 in spots.values():
        B[ci[first], n0] = np.nan; B[ci[mid], n0 + 1] = np.nan; B[ci[last], n0 + 2] = np.nan
        B[ci[mid], n0 + 3] = np.nan; B[ci[last], n0 + 3] = np.nan   # two NaN products in one column: the first wins
    with np.errstate(all="ignore"):
        assert np.all((v[rp[dead]:rp[dead + 1], None] * B[ci[rp[dead]:rp[dead + 1]]]) == -np.inf)
    a = Abi(sx, rp, ci, v, M, K)
    for reduce in OPS:
        wantC, wantA = ref_reduce(rp, ci, v, B, reduce)
        for r, ((first, mid, last), n0) in spots.items():
            assert np.all(np.isnan(wantC[r, n0:n0 + 4])) and list(wantA[r, n0:n0 + 4]) == [first, mid, last, mid]
        assert np.all(wantC[dead] == -np.inf) and np.all(wantA[dead] == rp[dead])
        C, arg, _, _ = a.forward(reduce, B)
        assert np.array_equal(arg, wantA), reduce
        assert bits_equal(C, wantC), reduce
    a.eng.close()


_torch_cpu = {}


def torch_cpu_reference(rp, ci, v, B, G, reduce, M, K):
    """torch's CPU torch.sparse.mm(A, B, reduce) and its autograd: (C, dB, dval), computed once per case"""
    import torch
    key = (reduce, B.shape[1])
    if key not in _torch_cpu:
        A = torch.sparse_csr_tensor(torch.from_numpy(rp.astype(np.int64)), torch.from_numpy(ci.astype(np.int64)), torch.from_numpy(v.copy()),
                                    size=(M, K)).requires_grad_()
        Bt = torch.from_numpy(B.copy()).requires_grad_()
        out = torch.sparse.mm(A, Bt, reduce)
        out.backward(torch.from_numpy(G))
        _torch_cpu[key] = (out.detach().numpy(), Bt.grad.numpy(), A.grad.values().numpy())
    return _torch_cpu[key]


def grad_inputs(N):
    rs, rp, ci, v, M, K = base_matrix(5)
    B, G = rand(rs, K, N), rand(rs, M, N)
    for reduce in OPS:
        assert tied_share(rp, ci, v, B, reduce) == 0.0
    return rs, rp, ci, v, M, K, B, G


@pytest.mark.parametrize("idx", [np.int64, np.int32])
@pytest.mark.parametrize("N", [20, 128])
def test_gradients_against_torch_cpu_autograd(sx, N, idx):
    import torch
    from sextans_amd import torch_op
    rs, rp, ci, v, M, K, B, G = grad_inputs(N)
    Gt = torch.from_numpy(G).cuda()
    for reduce in OPS:
        wantC, wantdB, wantdv = torch_cpu_reference(rp, ci, v, B, G, reduce, M, K)
        for grad_a, grad_b in ((False, True), (True, False), (True, True)):
            torch_op.clear_cache()
            A = make_A(rp, ci, v, M, K, grad=grad_a, dtype=idx)
            Bt = torch.from_numpy(B).cuda().requires_grad_(grad_b)
            out = torch_op.spmm_reduce(A, Bt, reduce)
            assert out.shape == (M, N) and out.dtype == torch.float32
            out.backward(Gt)
            info = torch_op.cache_info()
            assert info["engines_built"] == 1 and info["value_refreshes"] == 0, info
            assert bits_equal(out.detach().cpu().numpy(), wantC), reduce
            if grad_b:
                assert Bt.grad.shape == Bt.shape and Bt.grad.dtype == Bt.dtype
                assert _close(Bt.grad.cpu().numpy(), wantdB), (reduce, float(np.abs(Bt.grad.cpu().numpy() - wantdB).max()))
            else:
                assert Bt.grad is None
            if grad_a:
                assert A.grad.layout == torch.sparse_csr and A.grad.values().dtype == A.values().dtype
                assert A.grad.crow_indices().dtype == A.crow_indices().dtype
                assert _close(A.grad.values().cpu().numpy(), wantdv), (reduce, float(np.abs(A.grad.values().cpu().numpy() - wantdv).max()))
            else:
                assert A.grad is None
    torch_op.clear_cache()


def test_other_values_on_the_engine_between_forward_and_backward(sx):
    """the backward reads the values A had, through its own pointer: a spmm() with another value tensor on the same index tensors in
    between (a value refresh of the shared engine) changes nothing"""
    import torch
    from sextans_amd import torch_op
    rs, rp, ci, v, M, K, B, G = grad_inputs(20)
    Gt = torch.from_numpy(G).cuda()
    res = []
    for disturb in (False, True):
        torch_op.clear_cache()
        A = make_A(rp, ci, v, M, K, grad=True)
        Bt = torch.from_numpy(B).cuda().requires_grad_()
        out = torch_op.spmm_reduce(A, Bt, "amax")
        if disturb:
            A2 = torch.sparse_csr_tensor(A.crow_indices(), A.col_indices(), torch.from_numpy(rand(rs, len(ci))).cuda(), size=(M, K))
            torch_op.spmm(A2, Bt.detach())
            assert torch_op.cache_info() == {"engines_built": 1, "value_refreshes": 1, "entries": 1}
        out.backward(Gt)
        assert torch_op.cache_info()["engines_built"] == 1
        res.append([t.detach().cpu().numpy() for t in (out, Bt.grad, A.grad.values())])
    for x, y in zip(*res):
        assert same(x, y)
    torch_op.clear_cache()


def test_mean_sum_arg_and_errors(sx):
    import torch
    from sextans_amd import torch_op
    rs, rp, ci, v, M, K, B, G = grad_inputs(20)
    N = 20
    Gt = torch.from_numpy(G).cuda()
    torch_op.clear_cache()
    # mean against torch's CPU "mean", empty rows (0) and gradients included
    wantC, wantdB, wantdv = torch_cpu_reference(rp, ci, v, B, G, "mean", M, K)
    A = make_A(rp, ci, v, M, K, grad=True)
    Bt = torch.from_numpy(B).cuda().requires_grad_()
    out = torch_op.spmm_reduce(A, Bt, "mean")
    out.backward(Gt)
    outn = out.detach().cpu().numpy()
    empty = np.flatnonzero(np.diff(rp) == 0)
    assert len(empty) > 10 and np.all(outn[empty] == 0)
    assert _close(outn, wantC) and _close(Bt.grad.cpu().numpy(), wantdB) and _close(A.grad.values().cpu().numpy(), wantdv)
    # sum is spmm
    A0 = make_A(rp, ci, v, M, K)
    B0 = torch.from_numpy(B).cuda()
    assert same(torch_op.spmm_reduce(A0, B0, "sum").cpu().numpy(), torch_op.spmm(A0, B0).cpu().numpy())
    with pytest.raises(ValueError):
        torch_op.spmm_reduce(A0, B0, "max")
    with pytest.raises(ValueError):
        torch_op.spmm_reduce(A0, B0, "mean", return_arg=True)
    with pytest.raises(ValueError):
        torch_op.spmm_reduce(A0, B0, "sum", return_arg=True)
    # the winning entries; `fast` selects another engine, not another result
    for reduce in OPS:
        wC, wA = ref_reduce(rp, ci, v, B, reduce)
        C, arg = torch_op.spmm_reduce(A0, B0, reduce, return_arg=True)
        assert arg.dtype == torch.int32 and arg.shape == (M, N)
        assert bits_equal(C.cpu().numpy(), wC) and np.array_equal(arg.cpu().numpy(), wA)
        assert bits_equal(torch_op.spmm_reduce(A0, B0, reduce, fast=True).cpu().numpy(), wC)
        C, arg = torch_op.spmm_reduce(A, Bt, reduce, return_arg=True)     # on the autograd path too
        assert not arg.requires_grad and C.requires_grad
        assert bits_equal(C.detach().cpu().numpy(), wC) and np.array_equal(arg.cpu().numpy(), wA)
        # a B that is not contiguous, and N = 20 (no multiple of 8): the copy path, the values of the contiguous padded form
        Bp = np.zeros((K, 24), np.float32); Bp[:, :N] = B
        Cp = torch_op.spmm_reduce(A0, torch.from_numpy(Bp).cuda(), reduce).cpu().numpy()
        assert bits_equal(Cp[:, :N], wC)
        Bnc = torch.from_numpy(np.ascontiguousarray(Bp.T)).cuda().t()
        assert not Bnc.is_contiguous()
        assert bits_equal(torch_op.spmm_reduce(A0, Bnc, reduce).cpu().numpy(), Cp)
    torch_op.clear_cache()


def test_degenerate_matrices(sx):
    rs = np.random.RandomState(3)
    M, K, N = 5, 6, 16
    B, G = rand(rs, K, N), rand(rs, M, N)
    # no entry at all
    a = Abi(sx, np.zeros(M + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), M, K)
    for reduce in OPS:
        C, arg, _, _ = a.forward(reduce, B)
        assert np.all(C.view(np.uint32) == 0) and np.all(arg == -1)
    dB, _ = a.backward(B, np.full((M, N), -1, np.int32), G)
    assert np.all(dB == 0)
    a.eng.close()
    # entries in the last row only
    rp = np.array([0, 0, 0, 0, 0, 3], np.int32)
    ci = np.array([0, 2, 5], np.int32)
    v = rand(rs, 3)
    a = Abi(sx, rp, ci, v, M, K)
    for reduce in OPS:
        wantC, wantA = ref_reduce(rp, ci, v, B, reduce)
        C, arg, _, _ = a.forward(reduce, B)
        assert bits_equal(C, wantC) and np.array_equal(arg, wantA)
        assert np.all(C[:4].view(np.uint32) == 0) and np.all(arg[:4] == -1) and np.all(arg[4] >= 0)
        wdB, wdv = ref_grads(ci, v, B, wantA, G, K)
        dB, dv = a.backward(B, arg, G)
        assert np.all(dB[[1, 3, 4]] == 0) and _close(dB, wdB) and _close(dv, wdv)
        # an upstream gradient of zeros gives zeros
        dB, dv = a.backward(B, arg, np.zeros_like(G))
        assert np.all(dB == 0) and np.all(dv == 0)
    a.eng.close()


def test_reproducibility_and_capture(sx):
    import torch
    from sextans_amd import torch_op
    rs = np.random.RandomState(8)
    rp, ci, v, M, K = edge_pattern(rs)
    N = 16
    B, B2, G = rand(rs, K, N), rand(rs, K, N), rand(rs, M, N)
    Gt = torch.from_numpy(G).cuda()

    def eager(Bn):
        A = make_A(rp, ci, v, M, K, grad=True)
        Bt = torch.from_numpy(Bn).cuda().requires_grad_()
        out, arg = torch_op.spmm_reduce(A, Bt, "amax", return_arg=True)
        out.backward(Gt)
        return [t.detach().cpu().numpy() for t in (out, arg, Bt.grad, A.grad.values())]

    torch_op.clear_cache()
    first, second = eager(B), eager(B)
    for x, y in zip(first, second):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    want = eager(B2)
    assert not np.array_equal(want[0], first[0])

    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K, grad=True)
    Bt = torch.from_numpy(B).cuda().requires_grad_()

    def step():
        A.grad = None
        Bt.grad = None
        out, arg = torch_op.spmm_reduce(A, Bt, "amax", return_arg=True)
        out.backward(Gt)
        return out, arg

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                            # warm-up: engine, softmax tables, A^T and its tables
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, arg = step()
    assert torch_op.cache_info()["engines_built"] == 1
    with torch.no_grad():
        Bt.copy_(torch.from_numpy(B2).cuda())
    g.replay()
    torch.cuda.synchronize()
    got = [t.detach().cpu().numpy() for t in (out, arg, Bt.grad, A.grad.values())]
    for i, (x, y) in enumerate(zip(got, want)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), i
    torch_op.clear_cache()
