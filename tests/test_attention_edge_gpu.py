"""Edge features inside the fused attention (sextans_attention_edge_device / sextans_attention_edge_backward_device and
torch_op.sparse_attention_edge): k_e = K[c] + Ek[e], v_e = V[c] + Ev[e] per stored entry and head.  O and every gradient, dEk and dEv
included, against a per-entry float64 torch-autograd computation with the tolerance the fused attention is held to (_close, rtol 2e-4);
row lengths around every lane-group size and beyond the long-row threshold; bit ties to the plain entries; the shared dE store;
dropout; masks, empty rows and degenerate matrices; operand placement; determinism and a captured step; the torch op."""
import numpy as np
import pytest

from test_fused_attention_gpu import edge_pattern, rand, same
from test_torch_attention_gpu import make_A, pattern
from test_torch_autograd_gpu import _close

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
NAMES = ("O", "dQ", "dK", "dV", "dEk", "dEv", "db")


def reference(rp, ci, M, ops, G, scale, mult=None):
    """float64, entry by entry.  ops: dict Q (M, H, d), K (Kk, H, d), V (Kk, H, dv), Ek (nnz, H, d) or None, Ev (nnz, H, dv) or None,
    b (nnz,) or None; mult: (nnz, H) dropout multipliers or None.  -> dict of numpy: O, dQ, dK, dV, dEk, dEv, db (None where no operand)"""
    import torch
    rows = torch.from_numpy(np.repeat(np.arange(M), np.diff(rp))).cuda()
    cols = torch.from_numpy(ci.astype(np.int64)).cuda()
    t = {k: (torch.from_numpy(np.ascontiguousarray(x)).cuda().double().requires_grad_() if x is not None else None) for k, x in ops.items()}
    H, dv = ops["Q"].shape[1], ops["V"].shape[2]
    ke = t["K"][cols] + (t["Ek"] if t["Ek"] is not None else 0.0)
    ve = t["V"][cols] + (t["Ev"] if t["Ev"] is not None else 0.0)
    s = (t["Q"][rows] * ke).sum(-1)
    if t["b"] is not None:
        s = s + t["b"][:, None]
    s = s * scale
    idx = rows[:, None].expand(-1, H)
    m = torch.full((M, H), float("-inf"), dtype=torch.float64, device="cuda").scatter_reduce(0, idx, s.detach(), "amax")
    ex = torch.exp(s - m[rows])
    p = ex / torch.zeros((M, H), dtype=torch.float64, device="cuda").index_add(0, rows, ex)[rows]
    if mult is not None:
        p = p * torch.from_numpy(mult).cuda().double()
    O = torch.zeros((M, H, dv), dtype=torch.float64, device="cuda").index_add(0, rows, p[:, :, None] * ve)
    O.backward(torch.from_numpy(G).cuda().double())
    res = {"O": O.detach().cpu().numpy()}
    for k, name in (("Q", "dQ"), ("K", "dK"), ("V", "dV"), ("Ek", "dEk"), ("Ev", "dEv"), ("b", "db")):
        res[name] = t[k].grad.cpu().numpy() if t[k] is not None else None
    return res


class Abi:
    """one engine on a pattern; operands as numpy (rows, H, w), placed in device buffers with `pad` extra floats per row (NaN in the
    padding of the inputs, SENTINEL all over the outputs before the call)"""

    def __init__(self, sx, rp, ci, M, K, H, d, dv):
        import torch
        self.t, self.sx = torch, sx
        self.M, self.K, self.H, self.d, self.dv, self.nnz = M, K, H, d, dv, len(ci)
        self.rp, self.ci = torch.from_numpy(rp.astype(np.int32)).cuda(), torch.from_numpy(np.asarray(ci, np.int32)).cuda()
        self.val = torch.full((max(len(ci), 1),), float("nan"), device="cuda")   # A's own values are not read
        self.eng = sx.Engine(0)
        self.eng.set_matrix_csr_device(M, K, len(ci), self.rp.data_ptr(), self.ci.data_ptr(), self.val.data_ptr())

    def put(self, x, pad):
        if x is None:
            return None
        x = np.asarray(x, np.float32)
        w = int(np.prod(x.shape[1:], dtype=np.int64))
        buf = self.t.full((max(x.shape[0], 1), w + pad), float("nan"), device="cuda")
        if x.shape[0]:
            buf[:x.shape[0], :w] = self.t.from_numpy(np.ascontiguousarray(x.reshape(x.shape[0], w))).cuda()
        return buf

    def out(self, rows, w, pad, extra=0):
        return self.t.full((max(rows + extra, 1), w + pad), SENTINEL, device="cuda")

    def run(self, ops, G, scale, drop=None, pad=0, grads="kv", shared=False, plain=False, dbias=True, raw=False):
        """forward + backward.  grads: which of dEk ('k') and dEv ('v') are asked for; shared: one buffer for both (returned as dEk);
        plain: through sextans_attention_device / _backward_device (no E).  -> dict of numpy (rows, H, w), lse; raw: the buffers too"""
        t, H, d, dv, M, K, nnz = self.t, self.H, self.d, self.dv, self.M, self.K, self.nnz
        ptr = lambda x: x.data_ptr() if x is not None else None   # noqa: E731
        ld = lambda x, w: x.stride(0) if x is not None else H * w + pad   # noqa: E731
        Q, Kt, V, Ek, Ev = (self.put(ops[k], pad) for k in ("Q", "K", "V", "Ek", "Ev"))
        b = self.put(ops["b"], 0)
        Gd = self.put(G, pad)
        O, lse = self.out(M, H * dv, pad), self.out(M, H, 0)
        delta, dQ, dK, dV = self.out(M, H, 0), self.out(M, H * d, pad), self.out(K, H * d, pad), self.out(K, H * dv, pad)
        dEk = self.out(nnz, H * d, pad, extra=3) if ("k" in grads and Ek is not None) else None
        dEv = dEk if shared else self.out(nnz, H * dv, pad, extra=3) if ("v" in grads and Ev is not None) else None
        db = self.out(nnz, 1, 0) if (dbias and b is not None) else None
        stream = t.cuda.current_stream().cuda_stream
        head = (H, d, dv, scale, ptr(Q), ld(Q, d), ptr(Kt), ld(Kt, d), ptr(V), ld(V, dv))
        if plain:
            self.eng.attention_device(*head, ptr(b), ptr(O), ld(O, dv), ptr(lse), stream)
            self.fwd_kernel = self.eng.last_kernel()
            self.eng.attention_backward_device(*head, ptr(b), ptr(O), ld(O, dv), ptr(lse), ptr(Gd), ld(Gd, dv), ptr(delta), ptr(dQ), ld(dQ, d),
                                               ptr(dK), ld(dK, d), ptr(dV), ld(dV, dv), ptr(db), stream)
        else:
            edge = (ptr(Ek), ld(Ek, d), ptr(Ev), ld(Ev, dv))
            self.eng.attention_edge_device(*head, *edge, ptr(b), ptr(O), ld(O, dv), ptr(lse), drop, stream)
            self.fwd_kernel = self.eng.last_kernel()
            self.eng.attention_edge_backward_device(*head, *edge, ptr(b), ptr(O), ld(O, dv), ptr(lse), ptr(Gd), ld(Gd, dv), ptr(delta), ptr(dQ),
                                                    ld(dQ, d), ptr(dK), ld(dK, d), ptr(dV), ld(dV, dv), ptr(dEk), ld(dEk, d), ptr(dEv), ld(dEv, dv),
                                                    ptr(db), drop, stream)
        t.cuda.synchronize()
        bufs = dict(O=(O, M, dv), dQ=(dQ, M, d), dK=(dK, K, d), dV=(dV, K, dv), dEk=(dEk, nnz, d), dEv=(None if shared else dEv, nnz, dv))
        res = {k: (x[:n, :H * w].cpu().numpy().reshape(n, H, w) if x is not None else None) for k, (x, n, w) in bufs.items()}
        res["db"] = db[:nnz, 0].cpu().numpy() if db is not None else None
        res["lse"] = lse[:M].cpu().numpy()
        if raw:
            res["raw"] = {k: x.cpu().numpy() for k, (x, _, _) in bufs.items() if x is not None}
        return res


def operands(rs, M, K, nnz, H, d, dv, mode, bias):
    """mode: 'key', 'value', 'both' (two tensors) or 'shared' (one tensor on both sides, d == dv)"""
    ops = dict(Q=rand(rs, M, H, d), K=rand(rs, K, H, d), V=rand(rs, K, H, dv))
    ops["Ek"] = rand(rs, nnz, H, d) if mode != "value" else None
    ops["Ev"] = ops["Ek"] if mode == "shared" else rand(rs, nnz, H, dv) if mode != "key" else None
    ops["b"] = rand(rs, nnz) if bias else None
    return ops, rand(rs, M, H, dv)


def check(got, want, names=NAMES):
    for k in names:
        if want.get(k) is None:
            assert got.get(k) is None, k
            continue
        assert got[k].shape == want[k].shape, k
        assert np.all(np.isfinite(got[k])), k
        print(k, "max abs error", float(np.abs(got[k] - want[k]).max()), "of", float(np.abs(want[k]).max()))
        assert _close(got[k], want[k]), (k, float(np.abs(got[k] - want[k]).max()))


DIMS = [(1, 16, 16), (3, 8, 24), (2, 64, 64), (2, 20, 40), (1, 128, 128)]
# (one tensor on both sides has one width: "shared" where d == dv)
CASES = [(H, d, dv, mode) for H, d, dv in DIMS for mode in ("key", "value", "both", "shared") if mode != "shared" or d == dv]


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("H, d, dv, mode", CASES)
def test_against_float64(sx, H, d, dv, mode, bias):
    M, K = 300, 260
    rs, rp, ci, _ = pattern(31 + d, M, K, 9)
    dp, dvp = -(-d // 8) * 8, -(-dv // 8) * 8   # the C ABI takes multiples of 8: zero columns (the torch op pads the same way)
    ops, G = operands(rs, M, K, len(ci), H, d, dv, mode, bias)
    scale = 1.0 / np.sqrt(d) if d == 16 else 0.37
    want = reference(rp, ci, M, ops, G, scale)
    if mode == "shared":
        want["dEk"], want["dEv"] = want["dEk"] + want["dEv"], None   # the one tensor's gradient: both uses
    grow = lambda x, w: x if x is None or x.shape[2] == w else np.concatenate([x, np.zeros(x.shape[:2] + (w - x.shape[2],), np.float32)], 2)   # noqa: E731
    padded = dict(Q=grow(ops["Q"], dp), K=grow(ops["K"], dp), V=grow(ops["V"], dvp), Ek=grow(ops["Ek"], dp), Ev=grow(ops["Ev"], dvp), b=ops["b"])
    a = Abi(sx, rp, ci, M, K, H, dp, dvp)
    got = a.run(padded, grow(G, dvp), scale, shared=(mode == "shared"))
    assert a.eng.last_kernel() == "attention_edge_fused_backward" and a.fwd_kernel == "attention_edge_fused"
    widths = dict(O=dv, dQ=d, dK=d, dV=dv, dEk=d, dEv=dv)
    for k, w in widths.items():
        if got[k] is not None:
            assert np.all(got[k][:, :, w:] == 0), k   # the zero columns stay zero
            got[k] = got[k][:, :, :w]
    check(got, want)
    a.eng.close()


def test_row_length_edges_and_long_rows(sx):
    rs = np.random.RandomState(8)
    rp, ci, _, M, K = edge_pattern(rs)
    assert M < 3000 and np.count_nonzero(ci == 0) > 2048 and np.diff(rp).max() == 2500
    H, d = 2, 16
    ops, G = operands(rs, M, K, len(ci), H, d, d, "both", True)
    a = Abi(sx, rp, ci, M, K, H, d, d)
    got = a.run(ops, G, 0.25)
    assert a.fwd_kernel == "attention_edge_fused+long_rows"
    assert a.eng.last_kernel() == "attention_edge_fused_backward+long_rows"
    check(got, reference(rp, ci, M, ops, G, 0.25))
    ones = np.flatnonzero(np.diff(rp) == 1)   # a row of one entry: p = 1, O is the one rounded sum V[c] + Ev[e]
    assert len(ones) == 2101
    assert same(got["O"][ones], ops["V"][ci[rp[ones]]] + ops["Ev"][rp[ones]])
    a.eng.close()


def test_ties_to_the_plain_kernels(sx):
    M, K, H, d, dv = 300, 260, 2, 16, 24
    rs, rp, ci, _ = pattern(5, M, K, 9)
    nnz = len(ci)
    ops, G = operands(rs, M, K, nnz, H, d, dv, "both", True)
    a = Abi(sx, rp, ci, M, K, H, d, dv)
    names = ("O", "lse", "dQ", "dK", "dV", "db")
    plain = a.run(dict(ops, Ek=None, Ev=None), G, 0.3, plain=True)
    assert a.eng.last_kernel() == "attention_fused_backward"
    none = a.run(dict(ops, Ek=None, Ev=None), G, 0.3)   # both E NULL: the plain kernels themselves
    assert a.eng.last_kernel() == "attention_fused_backward"
    for k in names:
        assert same(none[k], plain[k]), k
    zero = dict(ops, Ek=np.zeros((nnz, H, d), np.float32), Ev=np.zeros((nnz, H, dv), np.float32))   # x + 0 = x: the same bits again
    got = a.run(zero, G, 0.3)
    assert a.eng.last_kernel() == "attention_edge_fused_backward"
    for k in names:
        assert same(got[k], plain[k]), k
    check(got, reference(rp, ci, M, zero, G, 0.3), ("dEk", "dEv"))
    for side in ("Ek", "Ev"):   # one side alone: the other side's arithmetic is the plain one
        one = a.run(dict(zero, **{side: None}), G, 0.3)
        for k in names:
            assert same(one[k], plain[k]), (side, k)
        other = "dEv" if side == "Ek" else "dEk"
        assert one["d" + side] is None and same(one[other], got[other])
    a.eng.close()


def test_shared_store(sx):
    M, K, H, d = 300, 260, 3, 24
    rs, rp, ci, _ = pattern(6, M, K, 9)
    ops, G = operands(rs, M, K, len(ci), H, d, d, "both", True)
    a = Abi(sx, rp, ci, M, K, H, d, d)
    two = a.run(ops, G, 0.3)
    one = a.run(ops, G, 0.3, shared=True)
    assert one["dEv"] is None
    assert same(one["dEk"], two["dEk"] + two["dEv"])   # (numpy float32: one rounded add per element)
    assert not same(one["dEk"], two["dEk"])
    for k in ("O", "lse", "dQ", "dK", "dV", "db"):
        assert same(one[k], two[k]), k
    for grads in ("k", "v", ""):   # gradients not asked for change nothing else
        part = a.run(ops, G, 0.3, grads=grads)
        for k in ("dQ", "dK", "dV", "db") + tuple("dE" + g for g in grads):
            assert same(part[k], two[k]), (grads, k)
    a.eng.close()


def test_dropout(sx):
    import torch
    M, K, H, d, dv, p, seed = 300, 260, 2, 16, 24, 0.5, 99
    rs, rp, ci, _ = pattern(7, M, K, 9)
    nnz = len(ci)
    ops, G = operands(rs, M, K, nnz, H, d, dv, "both", True)
    a = Abi(sx, rp, ci, M, K, H, d, dv)
    base = a.run(ops, G, 0.3)
    zero = a.run(ops, G, 0.3, drop=sx.api.Dropout(0.0, seed))
    assert a.eng.last_kernel() == "attention_edge_fused_backward"
    for k in NAMES + ("lse",):
        assert same(zero[k], base[k]), k
    drop = sx.api.Dropout(p, seed)
    mult = torch.empty((nnz, H), device="cuda")
    a.eng.dropout_mask_device(H, drop, mult.data_ptr(), torch.cuda.current_stream().cuda_stream)
    mult = mult.cpu().numpy()
    dropped = mult == 0
    assert 0.4 < dropped.mean() < 0.6 and np.all(mult[~dropped] == 2.0)
    got = a.run(ops, G, 0.3, drop=drop)
    assert a.fwd_kernel == "attention_edge_fused+dropout" and a.eng.last_kernel() == "attention_edge_fused_backward+dropout"
    check(got, reference(rp, ci, M, ops, G, 0.3, mult))
    assert same(got["lse"], base["lse"])               # the scores do not see the mask
    assert np.all(got["dEv"][dropped] == 0) and np.all(got["dEv"][~dropped][:, :8] != 0)
    a.eng.close()


def test_masks_empty_rows_and_degenerate_matrices(sx):
    from util import random_csr
    rs = np.random.RandomState(17)
    M, K, H, d, dv, scale = 400, 400, 2, 16, 24, 0.3
    rp, ci, _ = random_csr(rs, M, K - 20, 6, empty_frac=0.2)   # the last 20 columns have no entry
    lens = np.diff(rp)
    empty = np.flatnonzero(lens == 0)
    assert len(empty) > 20
    nnz = len(ci)
    ops, G = operands(rs, M, K, nnz, H, d, dv, "both", True)
    masked = rp[np.flatnonzero(lens >= 2)]   # rows of two or more entries: their first entry is masked out
    ops["b"][masked] = -np.inf
    a = Abi(sx, rp, ci, M, K, H, d, dv)
    got = a.run(ops, G, scale)
    # p = 0 there: dEk = (scale ds) * Q[r] and dEv = p * G[r] are zeros (by value: the one rounded multiply keeps the sign of Q / G)
    assert np.all(got["dEk"][masked] == 0) and np.all(got["dEv"][masked] == 0) and np.all(got["db"][masked] == 0)
    assert np.all(got["O"][empty].view(np.uint32) == 0) and np.all(got["lse"][empty] == -np.inf) and np.all(got["dQ"][empty] == 0)
    assert np.all(got["dK"][K - 20:] == 0) and np.all(got["dV"][K - 20:] == 0)
    check(got, reference(rp, ci, M, ops, G, scale))   # (exp(-inf) = 0 in float64 too; empty rows: zeros)
    a.eng.close()
    # no entries / no rows: OK, everything that has an element is filled
    for M0 in (M, 0):
        c = Abi(sx, np.zeros(M0 + 1, np.int32), np.zeros(0, np.int32), M0, K, H, d, dv)
        deg = dict(Q=rand(rs, M0, H, d), K=ops["K"], V=ops["V"], Ek=np.zeros((1, H, d), np.float32), Ev=np.zeros((1, H, dv), np.float32), b=None)
        c.nnz = 1   # (one row of E and dE behind the pointers: nothing of it is read or written)
        got = c.run(deg, rand(rs, M0, H, dv), scale)
        assert got["O"].shape == (M0, H, dv) and np.all(got["O"].view(np.uint32) == 0) and np.all(got["lse"] == -np.inf)
        assert all(np.all(got[k] == 0) for k in ("dQ", "dK", "dV"))
        assert np.all(got["dEk"] == SENTINEL) and np.all(got["dEv"] == SENTINEL)
        c.eng.close()


def test_operand_placement(sx):
    M, K, H, d, dv = 260, 240, 2, 16, 24
    rs, rp, ci, _ = pattern(51, M, K, 8)
    nnz = len(ci)
    ops, G = operands(rs, M, K, nnz, H, d, dv, "both", True)
    a = Abi(sx, rp, ci, M, K, H, d, dv)
    base = a.run(ops, G, 0.3)
    got = a.run(ops, G, 0.3, pad=12, raw=True)   # every leading dimension 12 floats wider, NaN behind the inputs' rows
    for k in NAMES + ("lse",):
        assert same(got[k], base[k]), k
    for k, w in (("O", dv), ("dQ", d), ("dK", d), ("dV", dv), ("dEk", d), ("dEv", dv)):
        buf = got["raw"][k]
        assert buf.shape[1] == H * w + 12 and np.all(buf[:, H * w:] == SENTINEL), k
    for k in ("dEk", "dEv"):
        buf = got["raw"][k]
        assert buf.shape[0] == nnz + 3 and np.all(buf[nnz:] == SENTINEL), k   # the rows beyond nnz
    a.eng.close()


def test_determinism_and_capture(sx):
    """two runs give equal bits; forward + backward captured into one graph with the dropout step bumped between replays"""
    import torch
    M, K, H, d, p, seed = 900, 900, 2, 16, 0.5, 11
    rs, rp, ci, _ = pattern(23, M, K, 10)
    nnz = len(ci)
    ops, Gn = operands(rs, M, K, nnz, H, d, d, "both", True)
    a = Abi(sx, rp, ci, M, K, H, d, d)
    first, second = a.run(ops, Gn, 0.25), a.run(ops, Gn, 0.25)
    for k in NAMES + ("lse",):
        assert same(first[k], second[k]), k
    dev = {k: torch.from_numpy(x.reshape(x.shape[0], -1)).cuda() for k, x in ops.items()}
    G = torch.from_numpy(Gn.reshape(M, -1)).cuda()
    w = H * d
    outs = dict(O=torch.empty(M, w), lse=torch.empty(M, H), delta=torch.empty(M, H), dQ=torch.empty(M, w), dK=torch.empty(K, w),
                dV=torch.empty(K, w), dEk=torch.empty(nnz, w), dEv=torch.empty(nnz, w), db=torch.empty(nnz))
    outs = {k: x.cuda() for k, x in outs.items()}
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    drop = sx.api.Dropout(p, seed, step.data_ptr())

    def both(stream):
        head = (H, d, d, 0.25, dev["Q"].data_ptr(), w, dev["K"].data_ptr(), w, dev["V"].data_ptr(), w, dev["Ek"].data_ptr(), w,
                dev["Ev"].data_ptr(), w, dev["b"].data_ptr(), outs["O"].data_ptr(), w, outs["lse"].data_ptr())
        a.eng.attention_edge_device(*head, drop, stream)
        a.eng.attention_edge_backward_device(*head, G.data_ptr(), w, outs["delta"].data_ptr(), outs["dQ"].data_ptr(), w, outs["dK"].data_ptr(), w,
                                             outs["dV"].data_ptr(), w, outs["dEk"].data_ptr(), w, outs["dEv"].data_ptr(), w, outs["db"].data_ptr(),
                                             drop, stream)

    def state():
        torch.cuda.synchronize()
        return {k: x.cpu().numpy().copy() for k, x in outs.items()}

    eager = []
    for k in (0, 1, 2):
        step.fill_(k)
        both(torch.cuda.current_stream().cuda_stream)   # (the first call builds the tables and A^T)
        eager.append(state())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        both(s.cuda_stream)
    for k in (0, 1, 2):
        for x in outs.values():
            x.fill_(SENTINEL)
        step.fill_(k)
        g.replay()
        got = state()
        for name in outs:
            assert same(got[name], eager[k][name]), (k, name)
    assert not same(eager[0]["O"], eager[1]["O"]) and not same(eager[1]["dEv"], eager[2]["dEv"])
    a.eng.close()


def test_torch_op(sx):
    import torch
    from sextans_amd import torch_op
    M, K, H, d, dv = 300, 260, 2, 16, 24
    rs, rp, ci, v = pattern(61, M, K, 9)
    nnz = len(ci)
    ops, Gn = operands(rs, M, K, nnz, H, d, dv, "both", True)
    ops["b"] = v
    leaf = lambda x: torch.from_numpy(x).cuda().requires_grad_()   # noqa: E731
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K, grad=True)
    Q, Kt, V, Ek = leaf(ops["Q"]), leaf(ops["K"]), leaf(ops["V"]), leaf(ops["Ek"])
    Ev = leaf(ops["Ev"].reshape(nnz, H * dv))   # (nnz, H dv) is accepted as (nnz, H, dv) is
    out = torch_op.sparse_attention_edge(A, Q, Kt, V, edge_key=Ek, edge_value=Ev, scale=0.3, bias=True)
    assert tuple(out.shape) == (M, H, dv)
    out.backward(torch.from_numpy(Gn).cuda())
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0, info
    assert A.grad.layout == torch.sparse_csr and tuple(Ev.grad.shape) == (nnz, H * dv)
    got = dict(O=out.detach().cpu().numpy(), dQ=Q.grad.cpu().numpy(), dK=Kt.grad.cpu().numpy(), dV=V.grad.cpu().numpy(), dEk=Ek.grad.cpu().numpy(),
               dEv=Ev.grad.cpu().numpy().reshape(nnz, H, dv), db=A.grad.values().cpu().numpy())
    check(got, reference(rp, ci, M, ops, Gn, 0.3))
    # one tensor on both sides: one gradient, the bits of the shared-store ABI call
    sh, Gs = operands(rs, M, K, nnz, H, d, d, "shared", False)
    Q, Kt, V, E = leaf(sh["Q"]), leaf(sh["K"]), leaf(sh["V"]), leaf(sh["Ek"])
    out = torch_op.sparse_attention_edge(A.detach(), Q, Kt, V, edge_key=E, edge_value=E)
    out.backward(torch.from_numpy(Gs).cuda())
    a = Abi(sx, rp, ci, M, K, H, d, d)
    want = a.run(sh, Gs, 0.25, shared=True)
    a.eng.close()
    assert same(out.detach().cpu().numpy(), want["O"]) and same(E.grad.cpu().numpy(), want["dEk"])
    assert same(Q.grad.cpu().numpy(), want["dQ"]) and same(Kt.grad.cpu().numpy(), want["dK"]) and same(V.grad.cpu().numpy(), want["dV"])
    # 2-D operands at H = 1, a key term alone, a head dimension that is no multiple of 8
    one, G1 = operands(rs, M, K, nnz, 1, 20, 12, "key", False)
    Q, Kt, V, E = leaf(one["Q"][:, 0]), leaf(one["K"][:, 0]), leaf(one["V"][:, 0]), leaf(one["Ek"][:, 0])
    out = torch_op.sparse_attention_edge(A.detach(), Q, Kt, V, edge_key=E, scale=0.37)
    assert tuple(out.shape) == (M, 12)
    out.backward(torch.from_numpy(G1[:, 0]).cuda())
    got = dict(O=out.detach().cpu().numpy()[:, None], dQ=Q.grad.cpu().numpy()[:, None], dK=Kt.grad.cpu().numpy()[:, None],
               dV=V.grad.cpu().numpy()[:, None], dEk=E.grad.cpu().numpy()[:, None])
    check(got, reference(rp, ci, M, one, G1, 0.37), ("O", "dQ", "dK", "dV", "dEk"))
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0, info
    with pytest.raises(ValueError):
        torch_op.sparse_attention_edge(A.detach(), Q, Kt, V, edge_key=E[:-1])
    with pytest.raises(ValueError):
        torch_op.sparse_attention_edge(A.detach(), Q, Kt, V, edge_key=E, dropout=1.0)
    torch_op.clear_cache()
