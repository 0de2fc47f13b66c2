"""spmm_edge_multi / spmm_edge_reduce and the C ABI under them (sextans_spmm_edge_multi_device_rm,
sextans_spmm_edge_multi_backward_device_rm): the sum, the sum of squares, the max and the min of the EDGE-FEATURE messages
m[e] = B[c] * E[e] | B[c] + E[e] | relu(B[c] + E[e]) | E[e] (one rounded fp32 operation, `messages` of test_spmm_edge_gpu.py) in one pass.
  The extrema and their args are bit-determined: compared EXACTLY with np.argmax / np.argmin over each row's fp32 message block (a NaN
wins, the first occurrence wins).
  The sums are compared with float64 sums of the fp32 messages under the worst case of an fp32 sum in ANY order of terms rounded once,
|got - want| <= (len + 1) 2^-23 sum |term| (within_bound of test_spmm_edge_gpu.py).
  The gradients are compared with a float64 evaluation of
      t_e[n]   = Gsum[r, n] + 2 m[e, n] Gsq[r, n] + (argmax[r, n] == e) Gmax[r, n] + (argmin[r, n] == e) Gmin[r, n]
      dB[c, n] = sum_e E[e, n] t_e[n] | t_e[n] | (B + E > 0) t_e[n]          dE[e, n] = t_e[n] B[c, n] | t_e[n] | (B + E > 0) t_e[n] | t_e[n]
under (terms + 4) 2^-23 sum |term|, the bound test_spmm_multi_gpu.py derives (grad_bound there): `terms` counts the terms added into the
element, + 4 covers the roundings inside a term.  Every comparison prints max err / bound; a value above 1 is a bug.
  With op MUL and E[e, :] = val[e] the messages are those of the scalar family; all six forward outputs and dB then have the BITS of
sextans_spmm_multi_device_rm / _backward_device_rm on the same engine (same product, same tile cap, same dealing; the entries in
flight differ, but a slot adds its entries one after the other whatever their number in flight)."""
import numpy as np
import pytest

import test_spmm_multi_gpu as multi
from test_fused_attention_gpu import edge_pattern, rand
from test_spmm_edge_gpu import EPS, OPS, messages, rows_of, scatter, within_bound
from test_spmm_multi_gpu import ALL, GRAD_SETS, POISON, VALUES, grad_bound, multi_matrix, raw_equal
from test_spmm_reduce_gpu import tie_inputs, tied_share
from test_torch_attention_gpu import make_A
from util import bits_equal as bits_equal_nan

pytestmark = pytest.mark.gpu

INVALID = 9   # SEXTANS_ERR_INVALID
WIDTHS = [8, 24, 64, 136]   # one tile, a partial tile, a full tile of 64, several tiles with a partial last one
SUBSETS = (("sum", "sumsq"), ("max", "min", "argmax", "argmin"), ("max", "min"), ("sum", "max", "argmax"), ("sumsq", "min"), ("sumsq",),
           ("min", "argmin"))   # the subsets test_spmm_multi_gpu.py asks for


class Abi(multi.Abi):
    """multi.Abi's engine (its forward / backward are the scalar family's) with the edge-feature entry points next to them"""

    def edge_forward(self, op, B, E, names=ALL, pad=0, concat=False):
        """as multi.Abi.forward: -> {name: (M, N) numpy} for `names` and {name: the whole buffer as int32}; B is not passed for copy"""
        t, api = self.t, self.sx.api
        N = E.shape[1]
        Bb = None
        if op != "copy":
            Bb = t.zeros((self.K, N + pad), device="cuda")
            Bb[:, :N] = t.from_numpy(B)
        Eb = t.zeros((max(self.nnz, 1), N + pad), device="cuda")
        Eb[:self.nnz, :N] = t.from_numpy(E)
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
        self.eng.spmm_edge_multi_device_rm(OPS[op], N, Bb.data_ptr() if Bb is not None else None, N + pad, Eb.data_ptr(), N + pad, o,
                                           t.cuda.current_stream().cuda_stream)
        t.cuda.synchronize()
        host = {name: b.cpu().numpy()[:self.M] for name, b in bufs.items()}
        out = {name: np.ascontiguousarray(host[name][:, view[name]]) for name in names}
        return {name: (a.view(np.float32) if name in VALUES else a) for name, a in out.items()}, host

    def edge_backward(self, op, B, E, args, grads, want_dB=True, want_dE=True):
        """args: {"max": argmax, "min": argmin}; grads: {name: (M, N) numpy} for the gradients that are given -> (dB, dE); dB is None
        for copy"""
        t, api = self.t, self.sx.api
        N = E.shape[1]
        dev = lambda x: t.from_numpy(np.ascontiguousarray(x)).cuda() if x.size else t.zeros(4, dtype=t.int32, device="cuda")   # noqa: E731
        want_dB = want_dB and op != "copy"
        Bb = dev(B) if op != "copy" else None
        keep = [dev(E)]
        g = api.MultiGrad()
        for name, G in grads.items():
            keep.append(dev(G))
            setattr(g, "d_g" + name, keep[-1].data_ptr())
            setattr(g, "ld_g" + name, N)
            if name in args:
                keep.append(dev(args[name]))
                setattr(g, "d_arg" + name, keep[-1].data_ptr())
        g.ld_arg = N
        dB = t.full((self.K, N), 7.0, device="cuda") if want_dB else None
        dE = t.full((max(self.nnz, 1), N), 7.0, device="cuda") if want_dE else None
        self.eng.spmm_edge_multi_backward_device_rm(OPS[op], N, Bb.data_ptr() if Bb is not None else None, N, keep[0].data_ptr(), N, g,
                                                    dB.data_ptr() if want_dB else None, N, dE.data_ptr() if want_dE else None, N,
                                                    t.cuda.current_stream().cuda_stream)
        t.cuda.synchronize()
        return (dB.cpu().numpy() if want_dB else None), (dE.cpu().numpy()[:self.nnz] if want_dE else None)


def ref_extrema(rp, m, reduce):
    """(C fp32, arg int32) by the rule: per row, np.argmax / np.argmin (NaN wins, the first occurrence wins) over the (entries, N) block of
    fp32 messages; an empty row gives +0 and -1"""
    M, N = len(rp) - 1, m.shape[1]
    C, arg = np.zeros((M, N), np.float32), np.full((M, N), -1, np.int32)
    pick = np.argmax if reduce == "amax" else np.argmin
    cols = np.arange(N)
    for r in range(M):
        b, e = int(rp[r]), int(rp[r + 1])
        if e > b:
            k = pick(m[b:e], axis=0)
            C[r], arg[r] = m[b + k, cols], b + k
    return C, arg


def tied_share_of(rp, m, reduce):
    """tied_share of test_spmm_reduce_gpu.py on message blocks: the share of the (row, column) positions of rows with two or more entries
    whose extreme is reached by more than one entry"""
    tied = total = 0
    for r in np.flatnonzero(np.diff(rp) >= 2):
        P = m[rp[r]:rp[r + 1]]
        ext = P.max(axis=0) if reduce == "amax" else P.min(axis=0)
        tied += int(np.count_nonzero((P == ext).sum(axis=0) > 1))
        total += P.shape[1]
    return tied / total


def reference(op, rp, ci, B, E):
    """the fp32 messages and, from them: float64 sum and sumsq with the sums of their terms' magnitudes, the extrema and args by the rule"""
    with np.errstate(all="ignore"):
        m = messages(op, B[ci] if op != "copy" else None, E)
        assert m.dtype == np.float32
        M, rows, m64 = len(rp) - 1, rows_of(rp), m.astype(np.float64)
        want = {"sum": scatter(rows, m64, M), "sumsq": scatter(rows, m64 * m64, M), "abs": scatter(rows, np.abs(m64), M)}
        want["max"], want["argmax"] = ref_extrema(rp, m, "amax")
        want["min"], want["argmin"] = ref_extrema(rp, m, "amin")
    return m, want


def check_forward(rp, m, want, got, what, one_bits=True):
    """the assertions on a full forward result `got` (all six outputs)"""
    lens = np.diff(rp)
    for name in ("max", "min"):
        assert raw_equal(got[name], want[name]) and np.array_equal(got["arg" + name], want["arg" + name]), (what, name)
    assert within_bound(got["sum"], want["sum"], want["abs"], lens, what + " sum")
    assert within_bound(got["sumsq"], want["sumsq"], want["sumsq"], lens, what + " sumsq")
    one = np.flatnonzero(lens == 1)            # a row of one entry: the message itself, its rounded square
    assert len(one) >= 3
    p = m[rp[one]]
    if one_bits:
        assert raw_equal(got["sum"][one], p) and raw_equal(got["sumsq"][one], p * p), what
    empty = np.flatnonzero(lens == 0)
    assert len(empty) > 10
    for name in VALUES:
        assert np.all(got[name][empty].view(np.uint32) == 0), (what, name)
    assert np.all(got["argmax"][empty] == -1) and np.all(got["argmin"][empty] == -1)


def ref_backward(op, rp, ci, B, E, args, grads, K):
    """float64 dB (K, N; None for copy) and dE (nnz, N) with fp32 messages, the sums of their terms' magnitudes and the number of terms
    added per element; ADD_RELU's mask is that of the fp32 sum (the sign of a rounded sum is the exact sum's)"""
    rows = rows_of(rp)
    e = np.arange(len(ci))[:, None]
    with np.errstate(all="ignore"):
        m = messages(op, B[ci] if op != "copy" else None, E).astype(np.float64)
    shape = m.shape
    terms = []
    if "sum" in grads:
        terms.append((grads["sum"].astype(np.float64)[rows], np.ones(shape, bool)))
    if "sumsq" in grads:
        terms.append((2.0 * m * grads["sumsq"].astype(np.float64)[rows], np.ones(shape, bool)))
    for name in ("max", "min"):
        if name in grads:
            won = args[name][rows] == e
            terms.append((np.where(won, grads[name].astype(np.float64)[rows], 0.0), won))
    t = sum(x for x, _ in terms)
    tabs = sum(np.abs(x) for x, _ in terms)
    cnt = sum(c.astype(np.int64) for _, c in terms)
    E64 = E.astype(np.float64)
    if op == "mul":
        B64 = B.astype(np.float64)[ci]
        fB, fE = E64, B64
    elif op == "add_relu":
        fB = fE = (B[ci] + E > 0).astype(np.float64)
    else:
        fB = fE = np.ones(shape)
    out = dict(dE=fE * t, dE_abs=np.abs(fE) * tabs, dE_cnt=cnt)
    if op != "copy":
        out.update(dB=scatter(ci, fB * t, K), dB_abs=scatter(ci, np.abs(fB) * tabs, K), dB_cnt=scatter(ci, cnt, K))
    return out


def operands(rs, op, K, nnz, N):
    """B, E: random floats; add_relu: B + E is negative for about three quarters of the messages (B - 0.7)"""
    B, E = rand(rs, K, N), rand(rs, nnz, N)
    if op == "add_relu":
        B = B - np.float32(0.7)
    return B, E


# ---- the forward on the C ABI -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("N", WIDTHS)
def test_forward_on_the_c_abi(sx, N, op):
    """every way of asking for the outputs gives the same bits; what is not asked for is not written"""
    rs, rp, ci, v, M, K = multi_matrix(5)
    B, E = operands(rs, op, K, len(ci), N)
    a = Abi(sx, rp, ci, v, M, K)
    full, _ = a.edge_forward(op, B, E)
    assert a.eng.last_kernel() == "spmm_edge_multi"
    m, want = reference(op, rp, ci, B, E)
    if op == "add_relu":   # a tie-heavy case of its own: most messages are +0, the first entry of the row must win
        share = tied_share_of(rp, m, "amin")
        print("add_relu: share of messages that are 0:", float(np.mean(m == 0)), "tied share of the min:", share)
        assert np.mean(m == 0) > 0.6 and share > 0.5 and tied_share_of(rp, m, "amax") > 0.02
    check_forward(rp, m, want, full, "%s N=%d" % (op, N))
    # padded leading dimensions: the padding is left alone
    got, host = a.edge_forward(op, B, E, pad=12)
    for name in ALL:
        assert raw_equal(got[name], full[name]) and np.all(host[name][:, N:] == POISON), name
    # the four values as slices of one (M, 4 N) buffer (+ padding)
    for pad in (0, 4):
        got, host = a.edge_forward(op, B, E, pad=pad, concat=True)
        for name in ALL:
            assert raw_equal(got[name], full[name]), name
        assert np.all(host["sum"][:, 4 * N:] == POISON)
    # each group alone, and a NULL output inside a group
    for names in SUBSETS:
        got, host = a.edge_forward(op, B, E, names=names)
        for name in ALL:
            if name in names:
                assert raw_equal(got[name], full[name]), (names, name)
            else:
                assert np.all(host[name] == POISON), (names, name)
    a.eng.close()


@pytest.mark.parametrize("op", ["mul", "add", "copy"])
def test_ties_and_signed_zeros(sx, op):
    """small integers: equal messages in a row and (mul) zeros of both signs -- the first entry wins, which is what the arg says, and
    every sum is exact.  mul with E[e, :] = val[e] has the products of tie_inputs / tied_share themselves"""
    rs, rp, ci, v, B, M, K = tie_inputs()
    N = B.shape[1]
    if op == "mul":
        E = np.repeat(v[:, None], N, 1)
        assert tied_share(rp, ci, v, B, "amax") >= 0.30 and tied_share(rp, ci, v, B, "amin") >= 0.30
    else:
        E = rs.randint(-2, 3, (len(ci), N)).astype(np.float32)
    m, want = reference(op, rp, ci, B, E)
    if op == "mul":
        assert np.any(m.view(np.uint32) == 0) and np.any(m.view(np.uint32) == 0x80000000)
    assert tied_share_of(rp, m, "amax") >= 0.30 and tied_share_of(rp, m, "amin") >= 0.30
    a = Abi(sx, rp, ci, v, M, K)
    got, _ = a.edge_forward(op, B, E)
    for name in ("max", "min"):
        assert raw_equal(got[name], want[name]) and np.array_equal(got["arg" + name], want["arg" + name]), name
    assert np.array_equal(got["sum"], want["sum"]) and np.array_equal(got["sumsq"], want["sumsq"])
    G = {name: rs.randint(-3, 4, (M, N)).astype(np.float32) for name in VALUES}
    args = {"max": want["argmax"], "min": want["argmin"]}
    for names in GRAD_SETS:
        grads = {name: G[name] for name in names}
        w = ref_backward(op, rp, ci, B, E, args, grads, K)
        dB, dE = a.edge_backward(op, B, E, args, grads)
        assert np.array_equal(dE, w["dE"]), names
        assert dB is None if op == "copy" else np.array_equal(dB, w["dB"]), names
    # the extrema's gradient alone: an entry that did not win gets nothing, although its message ties with the winner's
    _, dE = a.edge_backward(op, B, E, args, {"max": np.ones((M, N), np.float32)})
    e = np.arange(len(ci))[:, None]
    assert np.all(dE[want["argmax"][rows_of(rp)] != e] == 0)
    a.eng.close()


def test_infinities_and_nans(sx):
    """a NaN row and a +inf row of E: a NaN message wins both extrema, the sums are not finite exactly on the rows that own such an entry"""
    rs, rp, ci, v, M, K = multi_matrix(9)
    N = 24
    B, E = rand(rs, K, N), rand(rs, len(ci), N)
    rows = rows_of(rp)
    e_nan, e_inf = 40, len(ci) // 2
    assert rows[e_nan] != rows[e_inf]
    E[e_nan], E[e_inf] = np.nan, np.inf
    a = Abi(sx, rp, ci, v, M, K)
    for op in ("mul", "copy"):
        got, _ = a.edge_forward(op, np.abs(B) + np.float32(0.5), E)
        _, want = reference(op, rp, ci, np.abs(B) + np.float32(0.5), E)
        for name in ("max", "min"):
            assert bits_equal_nan(got[name], want[name]) and np.array_equal(got["arg" + name], want["arg" + name]), name
        owns = np.zeros(M, bool)
        owns[[rows[e_nan], rows[e_inf]]] = True
        for name in ("sum", "sumsq"):
            assert np.array_equal(~np.isfinite(got[name]), np.repeat(owns[:, None], N, 1)), name
        assert np.all(np.isnan(got["max"][rows[e_nan]])) and np.all(np.isnan(got["min"][rows[e_nan]]))
        assert np.all(got["argmax"][rows[e_nan]] == e_nan) and np.all(got["argmin"][rows[e_nan]] == e_nan)
    a.eng.close()


@pytest.mark.parametrize("N", WIDTHS)
def test_the_scalar_family_has_the_same_bits(sx, N):
    """op MUL with E[e, :] = val[e]: the six forward outputs and dB of sextans_spmm_multi_device_rm / _backward_device_rm, bit for bit"""
    rs, rp, ci, v, M, K = multi_matrix(6)
    B = rand(rs, K, N)
    E = np.ascontiguousarray(np.repeat(v[:, None], N, 1))
    G = {name: rand(rs, M, N) for name in VALUES}
    a = Abi(sx, rp, ci, v, M, K)
    scalar, _ = a.forward(B)
    assert a.eng.last_kernel() == "spmm_multi"
    edge, _ = a.edge_forward("mul", B, E)
    for name in ALL:
        assert raw_equal(edge[name], scalar[name]), name
    args = {"max": scalar["argmax"], "min": scalar["argmin"]}
    for names in GRAD_SETS:
        grads = {name: G[name] for name in names}
        dB_scalar, _ = a.backward(B, args, grads, want_dval=False)
        dB_edge, _ = a.edge_backward("mul", B, E, args, grads, want_dE=False)
        assert raw_equal(dB_edge, dB_scalar), names
    a.eng.close()


# ---- the backward on the C ABI ----------------------------------------------------------------------------------------------------------
def check_backward(a, op, rp, ci, B, E, args, G, what):
    rows = rows_of(rp)
    for names in GRAD_SETS:
        grads = {name: G[name] for name in names}
        w = ref_backward(op, rp, ci, B, E, args, grads, a.K)
        dB, dE = a.edge_backward(op, B, E, args, grads)
        assert grad_bound(dE, w["dE"], w["dE_abs"], w["dE_cnt"], "%s %s dE" % (what, "+".join(names)))
        # d_dE alone, d_dB alone: the same bits
        assert raw_equal(a.edge_backward(op, B, E, args, grads, want_dB=False)[1], dE), names
        if op == "copy":
            assert dB is None
        else:
            assert grad_bound(dB, w["dB"], w["dB_abs"], w["dB_cnt"], "%s %s dB" % (what, "+".join(names)))
            assert raw_equal(a.edge_backward(op, B, E, args, grads, want_dE=False)[0], dB), names
    if op in ("add", "copy"):   # t = Gsum, stored as it is
        _, dE = a.edge_backward(op, B, E, args, {"sum": G["sum"]})
        assert raw_equal(dE, G["sum"][rows]), op


@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("N", WIDTHS)
def test_backward_on_the_c_abi(sx, N, op):
    rs, rp, ci, v, M, K = multi_matrix(6)
    B, E = operands(rs, op, K, len(ci), N)
    G = {name: rand(rs, M, N) for name in VALUES}
    a = Abi(sx, rp, ci, v, M, K)
    got, _ = a.edge_forward(op, B, E)
    check_backward(a, op, rp, ci, B, E, {"max": got["argmax"], "min": got["argmin"]}, G, "%s N=%d" % (op, N))
    assert a.eng.last_kernel() == "spmm_edge_multi_backward"
    a.eng.close()


@pytest.mark.parametrize("op", ["mul", "add_relu"])
def test_long_rows_and_columns(sx, op):
    """a row of 2500 entries and a column of more than 2048: the workgroup kernels on A and on A^T"""
    rs = np.random.RandomState(8)
    rp, ci, v, M, K = edge_pattern(rs)
    N = 40
    assert M < 3000 and np.count_nonzero(ci == 0) > 2048 and np.diff(rp).max() == 2500
    B, E = operands(rs, op, K, len(ci), N)
    G = {name: rand(rs, M, N) for name in VALUES}
    a = Abi(sx, rp, ci, v, M, K)
    got, _ = a.edge_forward(op, B, E)
    assert a.eng.last_kernel() == "spmm_edge_multi+long_rows"
    m, want = reference(op, rp, ci, B, E)
    lens = np.diff(rp)
    for name in ("max", "min"):
        assert raw_equal(got[name], want[name]) and np.array_equal(got["arg" + name], want["arg" + name]), name
    assert within_bound(got["sum"], want["sum"], want["abs"], lens, "long sum")
    assert within_bound(got["sumsq"], want["sumsq"], want["sumsq"], lens, "long sumsq")
    for names in (("sum", "sumsq"), ("max", "min", "argmax", "argmin")):
        alone, _ = a.edge_forward(op, B, E, names=names)
        for name in names:
            assert raw_equal(alone[name], got[name]), name
    check_backward(a, op, rp, ci, B, E, {"max": got["argmax"], "min": got["argmin"]}, G, "long " + op)
    assert a.eng.last_kernel() == "spmm_edge_multi_backward+long_rows"
    a.eng.close()


def test_required_operands_and_degenerate_matrices(sx):
    """with nnz > 0: E always, B unless COPY -- refused before the device is touched; no entry / no row at all: zeros and -1"""
    import torch
    api = sx.api
    rs, rp, ci, v, M, K = multi_matrix(5)
    N = 16
    a = Abi(sx, rp, ci, v, M, K)
    buf = torch.zeros((max(len(ci), M, K), N), device="cuda")
    iarg = torch.zeros((M, N), dtype=torch.int32, device="cuda")
    p = buf.data_ptr()
    o = api.MultiOut(d_sum=p, ld_sum=N)
    g = api.MultiGrad(d_gsum=p, ld_gsum=N, d_gmax=p, ld_gmax=N, d_argmax=iarg.data_ptr(), ld_arg=N)
    for op, dB, dE in ((api.EDGE_MUL, None, p), (api.EDGE_MUL, p, None), (api.EDGE_ADD, p, None), (api.EDGE_COPY, None, None)):
        with pytest.raises(api.SextansError) as ei:
            a.eng.spmm_edge_multi_device_rm(op, N, p, N, None, N, o)                       # no E
        assert ei.value.code == INVALID
        with pytest.raises(api.SextansError) as ei:
            a.eng.spmm_edge_multi_backward_device_rm(op, N, p, N, None, N, g, dB, N, dE if dE or dB else p, N)
        assert ei.value.code == INVALID
        if op != api.EDGE_COPY:
            with pytest.raises(api.SextansError) as ei:
                a.eng.spmm_edge_multi_device_rm(op, N, None, N, p, N, o)                   # no B
            assert ei.value.code == INVALID
            with pytest.raises(api.SextansError) as ei:
                a.eng.spmm_edge_multi_backward_device_rm(op, N, None, N, p, N, g, dB, N, dE, N)
            assert ei.value.code == INVALID
    a.eng.close()
    K = 6
    for M in (5, 0):                                   # no entry at all; no row at all
        B, E, G = rand(rs, K, N), np.zeros((0, N), np.float32), rand(rs, M, N)
        a = Abi(sx, np.zeros(M + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), M, K)
        got, _ = a.edge_forward("mul", B, E)
        for name in VALUES:
            assert got[name].shape == (M, N) and np.all(got[name].view(np.uint32) == 0), name
        assert np.all(got["argmax"] == -1) and np.all(got["argmin"] == -1)
        none = np.full((M, N), -1, np.int32)
        dB, _ = a.edge_backward("mul", B, E, {"max": none, "min": none}, {name: G for name in VALUES})
        assert dB.shape == (K, N) and np.all(dB == 0)
        a.eng.close()


# ---- torch ------------------------------------------------------------------------------------------------------------------------------
def run_torch(fn, rp, ci, M, K, B, E, Gt):
    """fn(A, Bt, Et) -> out; -> out, dB, dE as numpy (B None: copy)"""
    import torch
    A = make_A(rp, ci, np.ones(len(ci), np.float32), M, K)
    Bt = torch.from_numpy(B).cuda().requires_grad_() if B is not None else None
    Et = torch.from_numpy(E).cuda().requires_grad_()
    out = fn(A, Bt, Et)
    out.backward(Gt)
    return [t.detach().cpu().numpy() if t is not None else None for t in (out, Bt.grad if Bt is not None else None, Et.grad)]


def test_reproducibility_and_capture(sx):
    """the same bits on every run, and under hipGraph capture and replay the bits of the eager call (long rows and a long column)"""
    import torch
    from sextans_amd import torch_op
    rs = np.random.RandomState(8)
    rp, ci, v, M, K = edge_pattern(rs)
    N = 16
    nnz = len(ci)
    B, E, B2, E2, G = rand(rs, K, N), rand(rs, nnz, N), rand(rs, K, N), rand(rs, nnz, N), rand(rs, M, 4 * N)
    Gt = torch.from_numpy(G).cuda()
    aggr = ("mean", "max", "min", "std")
    fn = lambda A, Bt, Et: torch_op.spmm_edge_multi(A, Bt, Et, "mul", aggr)   # noqa: E731

    torch_op.clear_cache()
    first, second = run_torch(fn, rp, ci, M, K, B, E, Gt), run_torch(fn, rp, ci, M, K, B, E, Gt)
    for x, y in zip(first, second):
        assert raw_equal(x, y)
    want = run_torch(fn, rp, ci, M, K, B2, E2, Gt)
    assert not np.array_equal(want[0], first[0])

    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    Bt, Et = torch.from_numpy(B).cuda().requires_grad_(), torch.from_numpy(E).cuda().requires_grad_()

    def step():
        Bt.grad = None
        Et.grad = None
        out = fn(A, Bt, Et)
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
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0, info
    with torch.no_grad():
        Bt.copy_(torch.from_numpy(B2).cuda())
        Et.copy_(torch.from_numpy(E2).cuda())
    g.replay()
    torch.cuda.synchronize()
    got = [t.detach().cpu().numpy() for t in (out, Bt.grad, Et.grad)]
    for i, (x, y) in enumerate(zip(got, want)):
        assert raw_equal(x, y), i
    torch_op.clear_cache()


def torch_reference(op, rp, ci, B, E, G, aggr, eps, M):
    """float64 CPU torch: the messages materialised, index_add / scatter_reduce, the var / std formulas of spmm_multi, autograd
    -> out, dB (None for copy), dE, the aggregates by name"""
    import torch
    rows = torch.from_numpy(rows_of(rp).astype(np.int64))
    col = torch.from_numpy(ci.astype(np.int64))
    Bt = torch.from_numpy(B.astype(np.float64)).requires_grad_() if op != "copy" else None
    Et = torch.from_numpy(E.astype(np.float64)).requires_grad_()
    N = E.shape[1]
    P = Bt[col] * Et if op == "mul" else Bt[col] + Et if op == "add" else torch.relu(Bt[col] + Et) if op == "add_relu" else Et * 1.0
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
    return out.detach().numpy(), (Bt.grad.numpy() if Bt is not None else None), Et.grad.numpy(), {k: t.detach().numpy() for k, t in raw.items()}


def torch_operands(rs, op, K, nnz, N):
    """random floats; add_relu: B + E > 0 everywhere (B + 2.5), or its zeros would tie and torch would split their gradient"""
    B, E = rand(rs, K, N), rand(rs, nnz, N)
    return (B + np.float32(2.5) if op == "add_relu" else B), E


@pytest.mark.parametrize("aggr", [("mean", "max", "min", "std"), ("sum", "var", "min")])
@pytest.mark.parametrize("N", [12, 16])
@pytest.mark.parametrize("op", list(OPS))
def test_torch_op_against_float64_composition(sx, op, N, aggr):
    """values and the gradients of B and E against the composition torch offers (the messages materialised, index_add, scatter_reduce,
    autograd), in float64 on the CPU, under the bounds test_spmm_multi_gpu.py derives for spmm_multi's elementwise ops (value_bounds,
    raw_gradients there) on top of the kernels' own; N = 12 takes the padding path"""
    import torch
    from sextans_amd import torch_op
    rs, rp, ci, _, M, K = multi_matrix(5)
    nnz = len(ci)
    B, E = torch_operands(rs, op, K, nnz, N)
    G = rand(rs, M, len(aggr) * N)
    m, ref = reference(op, rp, ci, B, E)
    tied = tied_share_of(rp, m, "amax"), tied_share_of(rp, m, "amin")
    print("tied share of the max and of the min:", tied)
    assert tied == (0.0, 0.0)   # (torch splits a tie's gradient)
    eps = 1e-5
    wout, wdB, wdE, raw = torch_reference(op, rp, ci, B, E, G, aggr, eps, M)
    b = multi.value_bounds(rp, raw, ref["abs"])
    gr, ge = multi.raw_gradients(aggr, G, rp, raw, b)
    present = {name: gr[name] for name in VALUES if any(name in torch_op._MULTI_NEEDS[x] for x in aggr)}
    w = ref_backward(op, rp, ci, B, E, {"max": ref["argmax"], "min": ref["argmin"]}, present, K)
    rows = rows_of(rp)
    et = ge["sum"][rows] + 2 * np.abs(m.astype(np.float64)) * ge["sumsq"][rows]   # the error of t_e from the raw gradients' errors
    fB = np.abs(E.astype(np.float64)) if op == "mul" else np.ones(m.shape)        # |d message / d B|, |d message / d E| at most
    fE = np.abs(B.astype(np.float64))[ci] if op == "mul" else np.ones(m.shape)
    Gt = torch.from_numpy(G).cuda()
    Bn = B if op != "copy" else None
    torch_op.clear_cache()
    o, dB, dE = run_torch(lambda A, Bt, Et: torch_op.spmm_edge_multi(A, Bt, Et, op, aggr, eps=eps), rp, ci, M, K, Bn, E, Gt)
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0, info
    assert o.shape == (M, len(aggr) * N) and o.dtype == np.float32
    for j, name in enumerate(aggr):
        got, want = o[:, j * N:(j + 1) * N], wout[:, j * N:(j + 1) * N]
        if name in ("max", "min"):     # rounding is monotone: the fp32 extreme of the fp32 messages is the rounded float64 extreme
            assert raw_equal(got, want.astype(np.float32)) and raw_equal(got, ref[name]), name
            continue
        err = np.abs(got.astype(np.float64) - want)
        ok = b[name] > 0
        print(op, aggr, N, name, "max err / bound", float((err[ok] / b[name][ok]).max()))
        assert np.all(err <= b[name]), name
    assert dE.shape == E.shape and dE.dtype == np.float32
    assert grad_bound(dE, wdE, w["dE_abs"], w["dE_cnt"], "%s %s N=%d dE" % (op, aggr, N), extra=fE * et)
    if op == "copy":
        assert dB is None
    else:
        assert dB.shape == B.shape and dB.dtype == np.float32
        assert grad_bound(dB, wdB, w["dB_abs"], w["dB_cnt"], "%s %s N=%d dB" % (op, aggr, N), extra=scatter(ci, fB * et, K))
    # only the gradient that is asked for is computed; without autograd, and `fast`: the same bits
    A = make_A(rp, ci, np.ones(nnz, np.float32), M, K)
    Bt, Et = (torch.from_numpy(B).cuda() if op != "copy" else None), torch.from_numpy(E).cuda()
    if op != "copy":
        Bg = Bt.clone().requires_grad_()
        out = torch_op.spmm_edge_multi(A, Bg, Et, op, aggr, eps=eps)
        out.backward(Gt)
        assert raw_equal(Bg.grad.cpu().numpy(), dB) and raw_equal(out.detach().cpu().numpy(), o)
    with torch.no_grad():
        assert raw_equal(torch_op.spmm_edge_multi(A, Bt, Et, op, aggr, eps=eps).cpu().numpy(), o)
        assert raw_equal(torch_op.spmm_edge_multi(A, Bt, Et, op, aggr, eps=eps, fast=True).cpu().numpy(), o)
    torch_op.clear_cache()


@pytest.mark.parametrize("reduce", ["amax", "amin"])
@pytest.mark.parametrize("N", [12, 16])
@pytest.mark.parametrize("op", list(OPS))
def test_spmm_edge_reduce_against_float64_composition(sx, op, N, reduce):
    import torch
    from sextans_amd import torch_op
    rs, rp, ci, _, M, K = multi_matrix(7)
    nnz = len(ci)
    B, E = torch_operands(rs, op, K, nnz, N)
    G = rand(rs, M, N)
    name = "max" if reduce == "amax" else "min"
    m, ref = reference(op, rp, ci, B, E)
    tied = tied_share_of(rp, m, reduce)
    print("tied share:", tied)
    assert tied == 0.0
    wout, wdB, wdE, _ = torch_reference(op, rp, ci, B, E, G, (name,), 0.0, M)
    w = ref_backward(op, rp, ci, B, E, {name: ref["arg" + name]}, {name: G}, K)
    Gt = torch.from_numpy(G).cuda()
    Bn = B if op != "copy" else None
    torch_op.clear_cache()
    o, dB, dE = run_torch(lambda A, Bt, Et: torch_op.spmm_edge_reduce(A, Bt, Et, op, reduce), rp, ci, M, K, Bn, E, Gt)
    assert o.shape == (M, N) and raw_equal(o, ref[name]) and raw_equal(o, wout.astype(np.float32))
    assert grad_bound(dE, wdE, w["dE_abs"], w["dE_cnt"], "%s %s N=%d dE" % (op, reduce, N))
    if op != "copy":
        assert grad_bound(dB, wdB, w["dB_abs"], w["dB_cnt"], "%s %s N=%d dB" % (op, reduce, N))
    A = make_A(rp, ci, np.ones(nnz, np.float32), M, K)
    Bt, Et = (torch.from_numpy(B).cuda() if op != "copy" else None), torch.from_numpy(E).cuda()
    C, arg = torch_op.spmm_edge_reduce(A, Bt, Et, op, reduce, return_arg=True)
    assert C.shape == (M, N) and arg.shape == (M, N) and arg.dtype == torch.int32
    assert raw_equal(C.cpu().numpy(), o) and np.array_equal(arg.cpu().numpy(), ref["arg" + name])
    C2, arg2 = torch_op.spmm_edge_reduce(A, Bt, Et.clone().requires_grad_(), op, reduce, return_arg=True)
    assert raw_equal(C2.detach().cpu().numpy(), o) and np.array_equal(arg2.cpu().numpy(), ref["arg" + name]) and not arg2.requires_grad
    torch_op.clear_cache()


def test_torch_op_placement_and_errors(sx):
    import torch
    from sextans_amd import torch_op
    rs, rp, ci, v, M, K = multi_matrix(5)
    N = 16
    nnz = len(ci)
    B, E = rand(rs, K, N), rand(rs, nnz, N)
    torch_op.clear_cache()
    A, Bt, Et = make_A(rp, ci, v, M, K), torch.from_numpy(B).cuda(), torch.from_numpy(E).cuda()
    a = Abi(sx, rp, ci, v, M, K)
    full, _ = a.edge_forward("mul", B, E)
    a.eng.close()
    # the raw aggregates, written in place: the ABI's bits, in any order and next to derived ones
    out = torch_op.spmm_edge_multi(A, Bt, Et, "mul", ("min", "sumsq", "max", "sum")).cpu().numpy()
    for j, name in enumerate(("min", "sumsq", "max", "sum")):
        assert raw_equal(out[:, j * N:(j + 1) * N], full[name]), name
    mixed = torch_op.spmm_edge_multi(A, Bt, Et, "mul", ("mean", "sum", "std", "max")).cpu().numpy()
    assert raw_equal(mixed[:, N:2 * N], full["sum"]) and raw_equal(mixed[:, 3 * N:], full["max"])
    deg = np.maximum(np.diff(rp), 1).astype(np.float32)[:, None]
    assert np.allclose(mixed[:, :N], full["sum"] / deg, rtol=2 * EPS, atol=0)
    # N = 12 and operands that are not contiguous: the copy path, the same values
    got = torch_op.spmm_edge_multi(A, Bt[:, :12], Et[:, :12], "mul", ("sum", "max")).cpu().numpy()
    assert raw_equal(got[:, :12], full["sum"][:, :12]) and raw_equal(got[:, 12:], full["max"][:, :12])
    assert raw_equal(torch_op.spmm_edge_multi(A, Bt, Et, "mul", ["max"]).cpu().numpy(), full["max"])   # a single aggregate
    assert raw_equal(torch_op.spmm_edge_reduce(A, Bt, Et).cpu().numpy(), full["max"])
    assert raw_equal(torch_op.spmm_edge_reduce(A, Bt, Et, reduce="amin").cpu().numpy(), full["min"])
    # the misuse spmm_edge refuses
    for fn in (torch_op.spmm_edge_multi, torch_op.spmm_edge_reduce):
        with pytest.raises(ValueError):
            fn(A, Bt, Et, "div")
        with pytest.raises(ValueError):
            fn(A, None, Et, "mul")                 # B=None goes with copy only
        with pytest.raises(ValueError):
            fn(A, Bt, Et, "copy")
        with pytest.raises(ValueError):
            fn(A, Bt[:K - 1], Et)
        with pytest.raises(ValueError):
            fn(A, Bt, Et[:nnz - 1])
        with pytest.raises(ValueError):
            fn(A, Bt[:, :8], Et)
        with pytest.raises(ValueError):
            fn(A, Bt.reshape(K, 2, 8), Et.reshape(nnz, 2, 8))   # 2-D operands only
        with pytest.raises(TypeError):
            fn(A, Bt.cpu(), Et)
        with pytest.raises(TypeError):
            fn(A, Bt, Et.cpu())
        with pytest.raises(TypeError):
            fn(A.to_dense(), Bt, Et)
    for bad in ((), ("sum", "median"), ("max", "max"), ("amax",), "max"):
        with pytest.raises(ValueError):
            torch_op.spmm_edge_multi(A, Bt, Et, "mul", bad)
    for bad in ("sum", "mean", "max"):
        with pytest.raises(ValueError):
            torch_op.spmm_edge_reduce(A, Bt, Et, "mul", bad)
    # spmm_edge keeps its refusals
    for bad in ("amax", "amin", "max"):
        with pytest.raises(ValueError):
            torch_op.spmm_edge(A, Bt, Et, "mul", reduce=bad)
    torch_op.clear_cache()
