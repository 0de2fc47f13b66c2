"""spmm_multi and the C ABI under it (sextans_spmm_multi_device_rm, sextans_spmm_multi_backward_device_rm): the sum, the sum of squares,
the max and the min of the messages p_e = fl(val[e] * B[c, :]) in one pass.
  The extrema and their args are bit-determined: compared EXACTLY with np.argmax / np.argmin over each row's fp32 product block
(ref_reduce of test_spmm_reduce_gpu.py) and with sextans_spmm_reduce_device_rm on the same engine.
  The sums are compared with float64 sums of the fp32 products under the worst case of an fp32 sum in ANY order of terms rounded once,
|got - want| <= (len + 1) 2^-23 sum |term| (within_bound of test_spmm_edge_gpu.py).
  The gradients are compared with a float64 evaluation of
      t_e[n] = Gsum[r, n] + 2 p_e[n] Gsq[r, n] + (argmax[r, n] == e) Gmax[r, n] + (argmin[r, n] == e) Gmin[r, n]
      dB[c, n] = sum_e val[e] t_e[n],   dval[e] = sum_n B[c, n] t_e[n]
under (terms + 4) 2^-23 sum |term|: `terms` counts the terms added into the element, + 4 covers the roundings inside a term (p_e, 2 p g,
the multiply by val or B) to first order.  Every comparison prints max err / bound; a value above 1 is a bug."""
import numpy as np
import pytest

from test_fused_attention_gpu import edge_pattern, rand
from test_spmm_edge_gpu import EPS, rows_of, scatter, within_bound
from test_spmm_reduce_gpu import ref_reduce, tie_inputs, tied_share
from test_torch_attention_gpu import make_A
from util import bits_equal as bits_equal_nan
from util import random_csr

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
VALUES = ("sum", "sumsq", "max", "min")
ARGS = ("argmax", "argmin")
ALL = VALUES + ARGS


def raw_equal(got, want):
    return got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


class Abi:
    """one engine on a matrix, operands as torch tensors, the entry points called through api.Engine"""

    def __init__(self, sx, rp, ci, v, M, K):
        import torch
        self.t, self.sx = torch, sx
        self.M, self.K, self.nnz = M, K, len(ci)
        self.rp, self.ci = torch.from_numpy(rp.astype(np.int32)).cuda(), torch.from_numpy(ci.astype(np.int32)).cuda()
        self.val = torch.zeros(max(self.nnz, 4), device="cuda")
        self.val[:self.nnz] = torch.from_numpy(np.asarray(v, np.float32))
        self.eng = sx.Engine(0)
        self.eng.set_matrix_csr_device(M, K, self.nnz, self.rp.data_ptr(), self.ci.data_ptr(), self.val.data_ptr())

    def forward(self, B, names=ALL, val=None, engine_values=False, pad=0, concat=False):
        """-> {name: (M, N) numpy (floats as float32, args as int32)} for `names`, and {name: the whole buffer as int32}: a name that is
        not asked for is passed as NULL and its buffer stays at POISON.  pad: extra columns of every buffer; concat: the four values are
        the column slices of ONE (M, 4 N) buffer"""
        t, api = self.t, self.sx.api
        N = B.shape[1]
        Bb = t.zeros((self.K, N + pad), device="cuda")
        Bb[:, :N] = t.from_numpy(B)
        rows = max(self.M, 1)
        o = api.MultiOut()
        bufs, view = {}, {}
        if concat:
            whole = t.full((rows, 4 * N + pad), POISON, dtype=t.int32, device="cuda")
        for j, name in enumerate(ALL):
            if concat and name in VALUES:
                bufs[name], ptr, ld = whole, whole.data_ptr() + 4 * N * j, 4 * N + pad
                view[name] = slice(j * N, (j + 1) * N)
            else:
                bufs[name] = t.full((rows, N + pad), POISON, dtype=t.int32, device="cuda")
                ptr, ld = bufs[name].data_ptr(), N + pad
                view[name] = slice(0, N)
            if name in names:
                setattr(o, "d_" + name, ptr)
            if name in VALUES:
                setattr(o, "ld_" + name, ld)
        o.ld_arg = N + pad
        vv = None if engine_values else (self.val if val is None else t.from_numpy(val).cuda())
        self.eng.spmm_multi_device_rm(N, vv.data_ptr() if vv is not None else None, Bb.data_ptr(), N + pad, o, t.cuda.current_stream().cuda_stream)
        t.cuda.synchronize()
        host = {name: b.cpu().numpy()[:self.M] for name, b in bufs.items()}
        out = {name: np.ascontiguousarray(host[name][:, view[name]]) for name in names}
        return {name: (a.view(np.float32) if name in VALUES else a) for name, a in out.items()}, host

    def reduce(self, op, B):
        """sextans_spmm_reduce_device_rm on the same engine -> (C, arg)"""
        t = self.t
        N = B.shape[1]
        Bt = t.from_numpy(B).cuda()
        C, arg = t.empty((max(self.M, 1), N), device="cuda"), t.empty((max(self.M, 1), N), dtype=t.int32, device="cuda")
        self.eng.spmm_reduce_device_rm(op, N, self.val.data_ptr(), Bt.data_ptr(), N, C.data_ptr(), N, arg.data_ptr(), N, t.cuda.current_stream().cuda_stream)
        t.cuda.synchronize()
        return C.cpu().numpy()[:self.M], arg.cpu().numpy()[:self.M]

    def backward(self, B, args, grads, want_dB=True, want_dval=True, val=None):
        """args: {"max": argmax, "min": argmin}; grads: {name: (M, N) numpy} for the gradients that are given -> (dB, dval)"""
        t, api = self.t, self.sx.api
        N = B.shape[1]
        dev = lambda x: t.from_numpy(np.ascontiguousarray(x)).cuda() if x.size else t.zeros(4, dtype=t.int32, device="cuda")   # noqa: E731
        keep = [dev(B)]
        g = api.MultiGrad()
        for name, G in grads.items():
            keep.append(dev(G))
            setattr(g, "d_g" + name, keep[-1].data_ptr())
            setattr(g, "ld_g" + name, N)
            if name in args:
                keep.append(dev(args[name]))
                setattr(g, "d_arg" + name, keep[-1].data_ptr())
        g.ld_arg = N
        vv = self.val if val is None else t.from_numpy(val).cuda()
        dB = t.full((self.K, N), 7.0, device="cuda") if want_dB else None
        dv = t.full((max(self.nnz, 4),), 7.0, device="cuda") if want_dval else None
        self.eng.spmm_multi_backward_device_rm(N, vv.data_ptr(), keep[0].data_ptr(), N, g, dB.data_ptr() if want_dB else None, N,
                                               dv.data_ptr() if want_dval else None, t.cuda.current_stream().cuda_stream)
        t.cuda.synchronize()
        return (dB.cpu().numpy() if want_dB else None), (dv.cpu().numpy()[:self.nnz] if want_dval else None)


def reference(rp, ci, v, B):
    """the fp32 products and, from them: float64 sum and sumsq with the sums of their terms' magnitudes, the extrema and args by the rule"""
    with np.errstate(all="ignore"):
        P = v[:, None].astype(np.float32) * B[ci].astype(np.float32)
        assert P.dtype == np.float32
        M, rows, P64 = len(rp) - 1, rows_of(rp), P.astype(np.float64)
        want = {"sum": scatter(rows, P64, M), "sumsq": scatter(rows, P64 * P64, M), "abs": scatter(rows, np.abs(P64), M)}
        want["max"], want["argmax"] = ref_reduce(rp, ci, v, B, "amax")
        want["min"], want["argmin"] = ref_reduce(rp, ci, v, B, "amin")
    return P, want


def check_forward(a, rp, ci, v, B, got, what):
    """the assertions on a full forward result `got` (all six outputs)"""
    P, want = reference(rp, ci, v, B)
    lens = np.diff(rp)
    for name in ("max", "min"):
        assert raw_equal(got[name], want[name]) and np.array_equal(got["arg" + name], want["arg" + name]), (what, name)
    assert within_bound(got["sum"], want["sum"], want["abs"], lens, what + " sum")
    assert within_bound(got["sumsq"], want["sumsq"], want["sumsq"], lens, what + " sumsq")
    one = np.flatnonzero(lens == 1)            # a row of one entry: the product itself, its rounded square
    assert len(one) >= 3
    p = P[rp[one]]
    assert raw_equal(got["sum"][one], p) and raw_equal(got["sumsq"][one], p * p), what
    empty = np.flatnonzero(lens == 0)
    assert len(empty) > 10
    for name in VALUES:
        assert np.all(got[name][empty].view(np.uint32) == 0), (what, name)
    assert np.all(got["argmax"][empty] == -1) and np.all(got["argmin"][empty] == -1)
    return want


def multi_matrix(seed):
    """400 x 300, Poisson 9, more than 10 empty rows, one row of 300, three rows cut down to one entry"""
    rs = np.random.RandomState(seed)
    M, K = 400, 300
    rp, ci, v = random_csr(rs, M, K, 9, empty_frac=0.1, long_rows=1)
    lens = np.diff(rp)
    cut = np.flatnonzero((lens >= 2) & (lens < 300))[[0, 7, -1]]
    keep = np.ones(len(ci), bool)
    for r in cut:
        keep[rp[r] + 1:rp[r + 1]] = False
    lens[cut] = 1
    rp2 = np.zeros(M + 1, np.int32); rp2[1:] = np.cumsum(lens)
    assert lens.max() == 300 and np.count_nonzero(lens == 0) > 10 and np.count_nonzero(lens == 1) >= 3
    return rs, rp2, ci[keep], v[keep], M, K


@pytest.mark.parametrize("N", [8, 24, 64, 136])
def test_forward_on_the_c_abi(sx, N):
    """one tile, a partial tile, several tiles; every way of asking for the outputs gives the same bits"""
    import torch
    rs, rp, ci, v, M, K = multi_matrix(5)
    B, v2 = rand(rs, K, N), rand(rs, len(ci))
    a = Abi(sx, rp, ci, v, M, K)
    full, _ = a.forward(B)
    assert a.eng.last_kernel() == "spmm_multi"
    check_forward(a, rp, ci, v, B, full, "N=%d" % N)
    for op, name in ((1, "max"), (2, "min")):          # the reduce kernel on the same engine: the same bits
        C, arg = a.reduce(op, B)
        assert raw_equal(full[name], C) and np.array_equal(full["arg" + name], arg), name
    # padded leading dimensions: the padding is left alone
    got, host = a.forward(B, pad=12)
    for name in ALL:
        assert raw_equal(got[name], full[name]) and np.all(host[name][:, N:] == POISON), name
    # the four values as slices of one (M, 4 N) buffer (+ padding)
    for pad in (0, 4):
        got, host = a.forward(B, pad=pad, concat=True)
        for name in ALL:
            assert raw_equal(got[name], full[name]), name
        assert np.all(host["sum"][:, 4 * N:] == POISON)
    # each group alone, and a NULL output inside a group: the others' bits do not change, what is not asked for is not written
    for names in (("sum", "sumsq"), ("max", "min", "argmax", "argmin"), ("max", "min"), ("sum", "max", "argmax"), ("sumsq", "min"), ("sumsq",),
                  ("min", "argmin")):
        got, host = a.forward(B, names=names)
        for name in ALL:
            if name in names:
                assert raw_equal(got[name], full[name]), (names, name)
            else:
                assert np.all(host[name] == POISON), (names, name)
    # d_val: NULL reads the engine's values; an explicit pointer to other values: the engine's own are not read
    got, _ = a.forward(B, engine_values=True)
    for name in ALL:
        assert raw_equal(got[name], full[name]), name
    got2, _ = a.forward(B, val=v2)
    check_forward(a, rp, ci, v2, B, got2, "N=%d other values" % N)
    nv = torch.from_numpy(v2).cuda()
    a.eng.update_values_device(nv.data_ptr(), torch.cuda.current_stream().cuda_stream)
    got, _ = a.forward(B, engine_values=True)
    for name in ALL:
        assert raw_equal(got[name], got2[name]), name
    a.eng.close()


def ref_backward(rp, ci, v, B, args, grads, K):
    """float64 dB (K, N) and dval (nnz) with fp32 p_e, the sums of their terms' magnitudes and the number of terms added per element"""
    rows = rows_of(rp)
    e = np.arange(len(ci))[:, None]
    P = (v[:, None].astype(np.float32) * B[ci].astype(np.float32)).astype(np.float64)
    terms = []
    if "sum" in grads:
        terms.append((grads["sum"].astype(np.float64)[rows], np.ones(P.shape, bool)))
    if "sumsq" in grads:
        terms.append((2.0 * P * grads["sumsq"].astype(np.float64)[rows], np.ones(P.shape, bool)))
    for name in ("max", "min"):
        if name in grads:
            won = args[name][rows] == e
            terms.append((np.where(won, grads[name].astype(np.float64)[rows], 0.0), won))
    t = sum(x for x, _ in terms)
    tabs = sum(np.abs(x) for x, _ in terms)
    cnt = sum(c.astype(np.int64) for _, c in terms)
    v64, B64 = v.astype(np.float64)[:, None], B.astype(np.float64)[ci]
    return dict(dB=scatter(ci, v64 * t, K), dB_abs=scatter(ci, np.abs(v64) * tabs, K), dB_cnt=scatter(ci, cnt, K),
                dv=(B64 * t).sum(1), dv_abs=(np.abs(B64) * tabs).sum(1), dv_cnt=cnt.sum(1))


def grad_bound(got, want, mags, cnt, what, extra=0.0):
    bound = (cnt + 4) * EPS * mags + extra
    err = np.abs(got.astype(np.float64) - want)
    ok = bound > 0
    print(what, "max |got - want|", float(err.max()) if err.size else 0.0, "max err / bound", float((err[ok] / bound[ok]).max()) if ok.any() else 0.0)
    return bool(np.all(err <= bound))


GRAD_SETS = (VALUES, ("sum", "sumsq"), ("max", "min"), ("sumsq",), ("sum", "min"))


def check_backward(a, rp, ci, v, B, args, G, what):
    for names in GRAD_SETS:
        grads = {name: G[name] for name in names}
        w = ref_backward(rp, ci, v, B, args, grads, a.K)
        dB, dv = a.backward(B, args, grads)
        assert grad_bound(dB, w["dB"], w["dB_abs"], w["dB_cnt"], "%s %s dB" % (what, "+".join(names)))
        assert grad_bound(dv, w["dv"], w["dv_abs"], w["dv_cnt"], "%s %s dval" % (what, "+".join(names)))
        # either of dB / dval alone: the same bits
        assert raw_equal(a.backward(B, args, grads, want_dval=False)[0], dB) and raw_equal(a.backward(B, args, grads, want_dB=False)[1], dv), names


@pytest.mark.parametrize("N", [8, 24, 64, 136])
def test_backward_on_the_c_abi(sx, N):
    rs, rp, ci, v, M, K = multi_matrix(6)
    B = rand(rs, K, N)
    G = {name: rand(rs, M, N) for name in VALUES}
    a = Abi(sx, rp, ci, v, M, K)
    got, _ = a.forward(B)
    check_backward(a, rp, ci, v, B, {"max": got["argmax"], "min": got["argmin"]}, G, "N=%d" % N)
    assert a.eng.last_kernel() == "spmm_multi_backward"
    a.eng.close()


@pytest.mark.parametrize("N", [16, 40])
def test_long_rows_and_columns(sx, N):
    rs = np.random.RandomState(8)
    rp, ci, v, M, K = edge_pattern(rs)
    assert M < 3000 and np.count_nonzero(ci == 0) > 2048 and np.diff(rp).max() == 2500
    B = rand(rs, K, N)
    G = {name: rand(rs, M, N) for name in VALUES}
    a = Abi(sx, rp, ci, v, M, K)
    got, _ = a.forward(B)
    assert a.eng.last_kernel() == "spmm_multi+long_rows"
    P, want = reference(rp, ci, v, B)
    lens = np.diff(rp)
    for name in ("max", "min"):
        assert raw_equal(got[name], want[name]) and np.array_equal(got["arg" + name], want["arg" + name]), name
    for op, name in ((1, "max"), (2, "min")):
        C, arg = a.reduce(op, B)
        assert raw_equal(got[name], C) and np.array_equal(got["arg" + name], arg), name
    assert within_bound(got["sum"], want["sum"], want["abs"], lens, "long sum")
    assert within_bound(got["sumsq"], want["sumsq"], want["sumsq"], lens, "long sumsq")
    one = np.flatnonzero(lens == 1)
    assert raw_equal(got["sum"][one], P[rp[one]]) and raw_equal(got["sumsq"][one], P[rp[one]] * P[rp[one]])
    for names in (("sum", "sumsq"), ("max", "min", "argmax", "argmin")):
        alone, _ = a.forward(B, names=names)
        for name in names:
            assert raw_equal(alone[name], got[name]), name
    check_backward(a, rp, ci, v, B, {"max": got["argmax"], "min": got["argmin"]}, G, "long N=%d" % N)
    assert a.eng.last_kernel() == "spmm_multi_backward+long_rows"
    a.eng.close()


def test_ties_and_signed_zeros(sx):
    """equal products in a row and zeros of both signs: the extrema's gradient goes to the FIRST entry only, which is what the arg says;
    small integers, so every sum is exact"""
    rs, rp, ci, v, B, M, K = tie_inputs()
    N = B.shape[1]
    prod = (v[:, None] * B[ci]).view(np.uint32)
    assert np.any(prod == 0) and np.any(prod == 0x80000000)
    assert tied_share(rp, ci, v, B, "amax") >= 0.30 and tied_share(rp, ci, v, B, "amin") >= 0.30
    a = Abi(sx, rp, ci, v, M, K)
    got, _ = a.forward(B)
    _, want = reference(rp, ci, v, B)
    for name in ("max", "min"):
        assert raw_equal(got[name], want[name]) and np.array_equal(got["arg" + name], want["arg" + name]), name
    assert np.array_equal(got["sum"], want["sum"]) and np.array_equal(got["sumsq"], want["sumsq"])
    G = {name: rs.randint(-3, 4, (M, N)).astype(np.float32) for name in VALUES}
    args = {"max": want["argmax"], "min": want["argmin"]}
    for names in GRAD_SETS:
        grads = {name: G[name] for name in names}
        w = ref_backward(rp, ci, v, B, args, grads, K)
        dB, dv = a.backward(B, args, grads)
        assert np.array_equal(dB, w["dB"]) and np.array_equal(dv, w["dv"]), names
    # the extrema's gradient alone: an entry that did not win gets nothing, although its product ties with the winner's
    dB, dv = a.backward(B, args, {"max": np.ones((M, N), np.float32)})
    winners = np.zeros(len(ci), bool)
    winners[want["argmax"][want["argmax"] >= 0]] = True
    assert np.all(dv[~winners] == 0)
    a.eng.close()


def test_infinities_and_nans(sx):
    rs, rp, ci, v, M, K = multi_matrix(9)
    N = 24
    B = rand(rs, K, N)
    k_nan, k_inf = 17, 123
    B[k_nan, :] = np.nan
    B[k_inf, :] = np.inf
    assert np.all(v != 0)
    a = Abi(sx, rp, ci, v, M, K)
    got, _ = a.forward(B)
    _, want = reference(rp, ci, v, B)
    for op, name in ((1, "max"), (2, "min")):
        C, arg = a.reduce(op, B)
        assert raw_equal(got[name], C) and np.array_equal(got["arg" + name], arg), name
        assert bits_equal_nan(got[name], want[name]) and np.array_equal(got["arg" + name], want["arg" + name]), name
    owns = np.zeros(M, bool)
    owns[rows_of(rp)[(ci == k_nan) | (ci == k_inf)]] = True
    assert 0 < owns.sum() < M
    for name in ("sum", "sumsq"):
        assert np.array_equal(~np.isfinite(got[name]), np.repeat(owns[:, None], N, 1)), name
    assert np.all(np.isnan(got["max"][rows_of(rp)[ci == k_nan]])) and np.all(np.isnan(got["min"][rows_of(rp)[ci == k_nan]]))
    a.eng.close()


def test_degenerate_matrices(sx):
    rs = np.random.RandomState(3)
    K, N = 6, 16
    for M in (5, 0):                                   # no entry at all; no row at all
        B, G = rand(rs, K, N), rand(rs, M, N)
        a = Abi(sx, np.zeros(M + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), M, K)
        got, _ = a.forward(B)
        for name in VALUES:
            assert got[name].shape == (M, N) and np.all(got[name].view(np.uint32) == 0), name
        assert np.all(got["argmax"] == -1) and np.all(got["argmin"] == -1)
        dB, _ = a.backward(B, {"max": np.full((M, N), -1, np.int32), "min": np.full((M, N), -1, np.int32)}, {name: G for name in VALUES})
        assert dB.shape == (K, N) and np.all(dB == 0)
        a.eng.close()


def test_empty_matrix_through_the_torch_op(sx):
    import torch
    from sextans_amd import torch_op
    torch_op.clear_cache()
    M, K, N = 7, 5, 16
    crow = torch.zeros(M + 1, dtype=torch.int64, device="cuda")
    A = torch.sparse_csr_tensor(crow, torch.zeros(0, dtype=torch.int64, device="cuda"), torch.zeros(0, device="cuda"), size=(M, K))
    B = torch.from_numpy(rand(np.random.RandomState(1), K, N)).cuda().requires_grad_()
    for n in (N, 12):
        Bn = B[:, :n]
        out = torch_op.spmm_multi(A, Bn, ("sum", "mean", "max", "min", "var", "std", "sumsq"), eps=1e-5)
        assert out.shape == (M, 7 * n)
        o = out.detach().cpu().numpy()
        assert np.all(o[:, :5 * n] == 0) and np.all(o[:, 6 * n:] == 0) and np.allclose(o[:, 5 * n:6 * n], np.sqrt(1e-5), rtol=2 * EPS, atol=0)
        B.grad = None
        out.sum().backward()
        assert np.all(B.grad.cpu().numpy() == 0)
    torch_op.clear_cache()


def test_reproducibility_and_capture(sx):
    import torch
    from sextans_amd import torch_op
    rs = np.random.RandomState(8)
    rp, ci, v, M, K = edge_pattern(rs)
    N = 16
    B, B2, G = rand(rs, K, N), rand(rs, K, N), rand(rs, M, 4 * N)
    Gt = torch.from_numpy(G).cuda()
    aggr = ("mean", "max", "min", "std")

    def eager(Bn):
        A = make_A(rp, ci, v, M, K, grad=True)
        Bt = torch.from_numpy(Bn).cuda().requires_grad_()
        out = torch_op.spmm_multi(A, Bt, aggr)
        out.backward(Gt)
        return [t.detach().cpu().numpy() for t in (out, Bt.grad, A.grad.values())]

    torch_op.clear_cache()
    first, second = eager(B), eager(B)
    for x, y in zip(first, second):
        assert raw_equal(x, y)
    want = eager(B2)
    assert not np.array_equal(want[0], first[0])

    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K, grad=True)
    Bt = torch.from_numpy(B).cuda().requires_grad_()

    def step():
        A.grad = None
        Bt.grad = None
        out = torch_op.spmm_multi(A, Bt, aggr)
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
        Bt.copy_(torch.from_numpy(B2).cuda())
    g.replay()
    torch.cuda.synchronize()
    got = [t.detach().cpu().numpy() for t in (out, Bt.grad, A.grad.values())]
    for i, (x, y) in enumerate(zip(got, want)):
        assert raw_equal(x, y), i
    torch_op.clear_cache()


# ---- torch_op.spmm_multi against a float64 composition on the CPU ---------------------------------------------------------------------
R = 8   # fp32 roundings on any path of the elementwise ops from an upstream gradient block to a raw gradient, at most


def torch_reference(rp, ci, v, B, G, aggr, eps, M):
    """float64 CPU torch: gather, index_add / scatter_reduce, the var / std formulas of spmm_multi, autograd -> out, dB, dval"""
    import torch
    rows = torch.from_numpy(rows_of(rp).astype(np.int64))
    col = torch.from_numpy(ci.astype(np.int64))
    vt = torch.from_numpy(v.astype(np.float64)).requires_grad_()
    Bt = torch.from_numpy(B.astype(np.float64)).requires_grad_()
    N = B.shape[1]
    P = vt[:, None] * Bt[col]
    idx = rows[:, None].expand(-1, N)
    zero = torch.zeros((M, N), dtype=torch.float64)
    raw = {"sum": zero.index_add(0, rows, P), "sumsq": zero.index_add(0, rows, P * P),
           "max": zero.scatter_reduce(0, idx, P, "amax", include_self=False), "min": zero.scatter_reduce(0, idx, P, "amin", include_self=False)}
    deg = torch.from_numpy(np.maximum(np.diff(rp), 1).astype(np.float64))[:, None]
    raw["mean"] = raw["sum"] / deg
    raw["var"] = raw["sumsq"] / deg - raw["mean"] ** 2
    raw["std"] = torch.sqrt(torch.relu(raw["var"]) + eps)
    out = torch.cat([raw[name] for name in aggr], 1)
    out.backward(torch.from_numpy(G.astype(np.float64)))
    return out.detach().numpy(), Bt.grad.numpy(), vt.grad.numpy(), {k: t.detach().numpy() for k, t in raw.items()}


def value_bounds(rp, raw, absS):
    """|fp32 aggregate - float64 aggregate| at most: the sums' (len + 1) 2^-23 sum |term| carried through the elementwise ops to first
    order, one 2^-23 per rounded operation.  mean = sum / deg: one more rounding.  var = sumsq / deg - mean^2: the error of sumsq / deg,
    2 |mean| times the error of mean, the roundings of the square and of the difference (each at most 2^-23 (q + m^2)), with
    q = sumsq / deg, m = sum |p| / deg >= |mean|.  std = sqrt(relu(var) + eps): the error of var over 2 std, two more roundings."""
    lens = np.diff(rp)[:, None].astype(np.float64)
    deg = np.maximum(lens, 1)
    q, m = raw["sumsq"] / deg, absS / deg
    b = {"sum": (lens + 1) * EPS * absS, "sumsq": (lens + 1) * EPS * raw["sumsq"], "max": 0 * q, "min": 0 * q}
    b["mean"] = (lens + 2) * EPS * m
    b["var"] = (lens + 2) * EPS * q + 2 * m * b["mean"] + 2 * EPS * (q + m * m)
    b["std"] = b["var"] / (2 * raw["std"]) + 2 * EPS * raw["std"]
    return b


def raw_gradients(aggr, G, rp, raw, b):
    """float64 upstream gradients of the kernel's raw outputs (what autograd hands to the one backward call), and bounds on the error
    of their fp32 counterparts: R roundings per path and the errors b of the forward values a path reads (mean, std)"""
    M, N = raw["sum"].shape
    deg = np.maximum(np.diff(rp), 1)[:, None].astype(np.float64)
    g = {name: np.zeros((M, N)) for name in VALUES}
    e = {name: np.zeros((M, N)) for name in ("sum", "sumsq")}
    mean, std, pos = raw["mean"], raw["std"], raw["var"] > 0
    for j, name in enumerate(aggr):
        Gj = G[:, j * N:(j + 1) * N].astype(np.float64)
        if name in VALUES:
            g[name] += Gj
        elif name == "mean":
            g["sum"] += Gj / deg
            e["sum"] += R * EPS * np.abs(Gj / deg)
        else:
            gv = Gj if name == "var" else np.where(pos, Gj / (2 * std), 0.0)          # the gradient of var
            ev = 0 * Gj if name == "var" else np.abs(gv) * (R * EPS + b["std"] / std)
            g["sumsq"] += gv / deg
            e["sumsq"] += (ev + R * EPS * np.abs(gv)) / deg
            g["sum"] += -2 * mean * gv / deg
            e["sum"] += 2 * (np.abs(mean) * (ev + R * EPS * np.abs(gv)) + np.abs(gv) * b["mean"]) / deg
    return g, e


@pytest.mark.parametrize("aggr", [("mean", "max", "min", "std"), ("sum", "var")])
@pytest.mark.parametrize("N", [20, 64])
def test_torch_op_against_float64_composition(sx, N, aggr):
    import torch
    from sextans_amd import torch_op
    rs, rp, ci, v, M, K = multi_matrix(5)
    B, G = rand(rs, K, N), rand(rs, M, len(aggr) * N)
    assert tied_share(rp, ci, v, B, "amax") == 0.0 and tied_share(rp, ci, v, B, "amin") == 0.0   # (torch splits a tie's gradient)
    eps = 1e-5
    wout, wdB, wdv, raw = torch_reference(rp, ci, v, B, G, aggr, eps, M)
    P, ref = reference(rp, ci, v, B)
    b = value_bounds(rp, raw, ref["abs"])
    gr, ge = raw_gradients(aggr, G, rp, raw, b)
    present = {name: gr[name] for name in VALUES if any(name in torch_op._MULTI_NEEDS[x] for x in aggr)}
    w = ref_backward(rp, ci, v, B, {"max": ref["argmax"], "min": ref["argmin"]}, present, K)
    rows = rows_of(rp)
    v64, B64, P64 = np.abs(v.astype(np.float64))[:, None], np.abs(B.astype(np.float64))[ci], np.abs(P.astype(np.float64))
    et = ge["sum"][rows] + 2 * P64 * ge["sumsq"][rows]            # the error of t_e from the raw gradients' errors
    Gt = torch.from_numpy(G).cuda()
    n = lambda t: t.detach().cpu().numpy()   # noqa: E731
    for grad_a, grad_b in ((True, True), (False, True), (True, False)):
        torch_op.clear_cache()
        A = make_A(rp, ci, v, M, K, grad=grad_a)
        Bt = torch.from_numpy(B).cuda().requires_grad_(grad_b)
        out = torch_op.spmm_multi(A, Bt, aggr, eps=eps)
        assert out.shape == (M, len(aggr) * N) and out.dtype == torch.float32
        out.backward(Gt)
        info = torch_op.cache_info()
        assert info["engines_built"] == 1 and info["value_refreshes"] == 0, info
        o = n(out)
        for j, name in enumerate(aggr):
            got, want = o[:, j * N:(j + 1) * N], wout[:, j * N:(j + 1) * N]
            if name in ("max", "min"):     # rounding is monotone: the fp32 extreme of the fp32 products is the rounded float64 extreme
                assert raw_equal(got, want.astype(np.float32)) and raw_equal(got, ref[name]), name
                continue
            err = np.abs(got.astype(np.float64) - want)
            ok = b[name] > 0
            print(aggr, N, name, "max err / bound", float((err[ok] / b[name][ok]).max()))
            assert np.all(err <= b[name]), name
        if grad_b:                                    # only the gradient that is asked for is computed
            assert Bt.grad.shape == Bt.shape and Bt.grad.dtype == torch.float32
            assert grad_bound(n(Bt.grad), wdB, w["dB_abs"], w["dB_cnt"], "%s N=%d dB" % (aggr, N), extra=scatter(ci, v64 * et, K))
        else:
            assert Bt.grad is None
        if grad_a:
            assert A.grad.layout == torch.sparse_csr and A.grad.values().dtype == torch.float32
            assert grad_bound(n(A.grad.values()), wdv, w["dv_abs"], w["dv_cnt"], "%s N=%d dA" % (aggr, N), extra=(B64 * et).sum(1))
        else:
            assert A.grad is None
    # without autograd, and `fast`: the same bits
    with torch.no_grad():
        A0 = make_A(rp, ci, v, M, K)
        assert raw_equal(n(torch_op.spmm_multi(A0, torch.from_numpy(B).cuda(), aggr, eps=eps)), o)
        assert raw_equal(n(torch_op.spmm_multi(A0, torch.from_numpy(B).cuda(), aggr, eps=eps, fast=True)), o)
    torch_op.clear_cache()


def test_torch_op_placement_and_errors(sx):
    import torch
    from sextans_amd import torch_op
    rs, rp, ci, v, M, K = multi_matrix(5)
    N = 16
    B = rand(rs, K, N)
    torch_op.clear_cache()
    A, Bt = make_A(rp, ci, v, M, K), torch.from_numpy(B).cuda()
    _, ref = reference(rp, ci, v, B)
    # the raw aggregates, written in place: the ABI's bits, in any order and next to derived ones
    out = torch_op.spmm_multi(A, Bt, ("min", "sumsq", "max", "sum")).cpu().numpy()
    a = Abi(sx, rp, ci, v, M, K)
    full, _ = a.forward(B)
    a.eng.close()
    for j, name in enumerate(("min", "sumsq", "max", "sum")):
        assert raw_equal(out[:, j * N:(j + 1) * N], full[name]), name
    mixed = torch_op.spmm_multi(A, Bt, ("mean", "sum", "std", "max")).cpu().numpy()
    assert raw_equal(mixed[:, N:2 * N], full["sum"]) and raw_equal(mixed[:, 3 * N:], full["max"])
    deg = np.maximum(np.diff(rp), 1).astype(np.float32)[:, None]
    assert np.allclose(mixed[:, :N], full["sum"] / deg, rtol=2 * EPS, atol=0)
    # N = 20 (no multiple of 8) and a B that is not contiguous: the copy path, the same values
    Bp = np.zeros((K, 24), np.float32); Bp[:, :20] = rand(rs, K, 20)
    want = torch_op.spmm_multi(A, torch.from_numpy(Bp).cuda(), ("sum", "max")).cpu().numpy()
    got = torch_op.spmm_multi(A, torch.from_numpy(Bp).cuda()[:, :20], ("sum", "max")).cpu().numpy()
    assert raw_equal(got[:, :20], want[:, :20]) and raw_equal(got[:, 20:], want[:, 24:44])
    Bnc = torch.from_numpy(np.ascontiguousarray(Bp.T)).cuda().t()
    assert not Bnc.is_contiguous() and raw_equal(torch_op.spmm_multi(A, Bnc, ("sum", "max")).cpu().numpy(), want)
    assert raw_equal(torch_op.spmm_multi(A, Bt, ["max"]).cpu().numpy(), full["max"])   # a single aggregate
    for bad in ((), ("sum", "median"), ("max", "max"), ("amax",), "max"):
        with pytest.raises(ValueError):
            torch_op.spmm_multi(A, Bt, bad)
    with pytest.raises(ValueError):
        torch_op.spmm_multi(A, Bt[:K - 1], ("sum",))
    with pytest.raises(TypeError):
        torch_op.spmm_multi(A, Bt.cpu(), ("sum",))
    with pytest.raises(TypeError):
        torch_op.spmm_multi(A.to_dense(), Bt, ("sum",))
    torch_op.clear_cache()
