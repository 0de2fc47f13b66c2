"""Per-head dot product on the pattern on the GPU through the C ABI (sextans_edge_dot_device / sextans_edge_dot_backward_device).
  Forward bits: S must equal a sequential numpy float32 loop (acc = acc + x * y, every product and sum rounded) AND, head by head,
sextans_sddmm_device_rm on the head's slice (alpha = 1, no vals_in), bit for bit -- on the 92-row pattern P of
test_pattern_dealing_gpu.py (rows of 2046 and 2048 entries that cross several 256-entry ranges, empty rows), on the 400 x 300 matrix of
the reduce tests, on tiny patterns of 1, 255, 256 and 257 entries whose first and last rows are empty, and on a pattern with a run of
more than 64 empty rows inside one range; heads 1, 3, 8 (8: a lane group keeps its head; 3: it changes every step), d 8 .. 128 (both
lane counts, every register depth of the X piece and the re-read variant are reached by 8, 16, 24, 64, 128 -- d = 24 is 3 chunks of 2
lanes, 128 is 8 chunks of 4).
  Integer operands in [-4, 4] on P and P^T: every dot is at most 128 * 16 = 2048 in magnitude and every gradient sum of at most 2600
terms of magnitude <= 16 an integer below 2^24, so S, dX and dY must EQUAL the int64 computation (the argument of test_edge_op_gpu.py).
  Backward: dX has the bits of sextans_score_attention_device(WEIGHT)'s O (S := Gs, V := Y), dY those of
sextans_score_attention_backward_device(WEIGHT)'s dV (S := Gs, G := X); both lie within (n + 2) 2^-24 sum |t_e| of a float64 reference
(test_edge_op_gpu.within_bound: derived there, not measured).  Pass selection, leading dimensions, special values, degenerate matrices,
determinism across runs, streams and a replayed graph."""
import numpy as np
import pytest

from test_edge_op_gpu import within_bound
from test_fused_attention_gpu import rand, same
from test_pattern_dealing_gpu import pat, rng
from test_spmm_edge_gpu import ints, rows_of
from test_spmm_reduce_gpu import POISON, Abi, base_matrix, bits_equal

pytestmark = pytest.mark.gpu

WEIGHT = 2   # SEXTANS_SCORE_WEIGHT
HEADS = [1, 3, 8]
DIMS = [8, 16, 24, 64, 128]
GRADS = ("dX", "dY")


def dot_ref(rp, ci, X, Y, H, d, dtype=np.float32):
    """(nnz, H) in `dtype`: the sequential loop over d, one rounded product and one rounded add per step"""
    x, y = X.astype(dtype).reshape(-1, H, d)[rows_of(rp)], Y.astype(dtype).reshape(-1, H, d)[ci]
    acc = np.zeros((len(ci), H), dtype)
    for n in range(d):
        acc = acc + x[:, :, n] * y[:, :, n]
    assert acc.dtype == dtype
    return acc


def grad_ref(rp, ci, X, Y, Gs, M, K, H, d, dtype=np.float64):
    """-> {dX (M, H d), dY (K, H d)} in `dtype`, {the sums of |t_e|}, {the entry counts}"""
    rows = rows_of(rp)
    g = Gs.astype(dtype)[:, :, None]
    tx = (g * Y.astype(dtype).reshape(K, H, d)[ci]).reshape(len(ci), H * d)
    ty = (g * X.astype(dtype).reshape(M, H, d)[rows]).reshape(len(ci), H * d)
    out, mags = {}, {}
    for name, idx, t, n in (("dX", rows, tx, M), ("dY", ci, ty, K)):
        out[name], mags[name] = np.zeros((n, H * d), dtype), np.zeros((n, H * d), dtype)
        np.add.at(out[name], idx, t)
        np.add.at(mags[name], idx, np.abs(t))
    return out, mags, {"dX": np.diff(rp), "dY": np.bincount(ci, minlength=K)}


def from_lens(rs, lens, K):
    """-> rp, ci, M, K: rows of `lens` entries, each row's columns sorted and distinct"""
    M = len(lens)
    rp = np.zeros(M + 1, np.int32); rp[1:] = np.cumsum(lens)
    ci = np.zeros(rp[-1], np.int32)
    for r, n in enumerate(lens):
        ci[rp[r]:rp[r + 1]] = np.sort(rs.choice(K, n, replace=False))
    return rp, ci, M, K


def small_patterns():
    """name -> (rp, ci, M, K): 1, 255, 256, 257 entries between two empty first rows and two empty last rows; a run of 70 and one of 130
    empty rows inside the first 256-entry range"""
    rs = np.random.RandomState(19)
    out = {}
    for nnz in (1, 255, 256, 257):
        a = nnz // 3
        out["nnz%d" % nnz] = from_lens(rs, [0, 0, a, 0, nnz - 2 * a, a, 0, 0], 300)
    out["empty_runs"] = from_lens(rs, [0] * 3 + [100] + [0] * 70 + [100] + [0] * 130 + [200, 57] + [0] * 4, 300)
    for rp, ci, M, K in out.values():
        assert rp[1] == 0 and rp[-2] == rp[-1]
    assert out["empty_runs"][0][-1] == 457
    return out


class DotAbi(Abi):
    """test_spmm_reduce_gpu.Abi's engine on a pattern (values 1: never read), the entry points called through api.Engine; X (M, H d),
    Y (K, H d), S and Gs (nnz, H) as numpy"""

    def __init__(self, sx, rp, ci, M, K):
        super().__init__(sx, rp, ci, np.ones(len(ci), np.float32), M, K)

    def dev(self, x, pad=0):
        """a numpy (rows, n) operand in a device buffer `pad` columns wider (NaN there), or None"""
        if x is None:
            return None
        tc = self.t
        buf = tc.full((max(x.shape[0], 1), x.shape[1] + pad), float("nan"), device="cuda")
        buf[:x.shape[0], :x.shape[1]] = tc.from_numpy(np.ascontiguousarray(x))
        return buf

    def stream(self):
        return self.t.cuda.current_stream().cuda_stream

    def fwd(self, X, Y, H, d, pad=(0, 0, 0)):
        """-> S as numpy float32 and the whole padded buffer as int32; pad: extra columns of the X / Y / S buffers"""
        tc = self.t
        Xb, Yb = self.dev(X, pad[0]), self.dev(Y, pad[1])
        Sb = tc.full((max(self.nnz, 1), H + pad[2]), POISON, dtype=tc.int32, device="cuda")
        self.eng.edge_dot_device(H, d, Xb.data_ptr(), H * d + pad[0], Yb.data_ptr(), H * d + pad[1], Sb.data_ptr(), H + pad[2], self.stream())
        tc.cuda.synchronize()
        Sn = Sb.cpu().numpy()[:self.nnz]
        return np.ascontiguousarray(Sn[:, :H]).view(np.float32), Sn

    def sddmm(self, X, Y, H, d):
        """(nnz, H): sextans_sddmm_device_rm head by head on the head's slice of the same buffers, alpha = 1, no vals_in"""
        tc = self.t
        Xb, Yb = self.dev(X), self.dev(Y)
        out = tc.full((H, -(-max(self.nnz, 4) // 4) * 4), 7.0, device="cuda")   # (every head's row 16-byte aligned)
        for h in range(H):
            self.eng.sddmm_device_rm(d, 1.0, Xb.data_ptr() + 4 * h * d, H * d, Yb.data_ptr() + 4 * h * d, H * d, 0.0, None,
                                     out[h].data_ptr(), self.stream())
        tc.cuda.synchronize()
        return np.ascontiguousarray(out.cpu().numpy()[:, :self.nnz].T)

    def bwd(self, X, Y, Gs, H, d, want=GRADS, pad=0, gpad=0):
        """-> {name: numpy} of both gradients, each in a buffer `pad` columns wider that held 7.0: the one not in `want` gets no pointer
        and must keep its 7.0; the operand a call does not read is not handed over"""
        tc = self.t
        Xb, Yb, Gb = self.dev(X if "dY" in want else None), self.dev(Y if "dX" in want else None), self.dev(Gs, gpad)
        buf = {"dX": tc.full((max(self.M, 1), H * d + pad), 7.0, device="cuda"), "dY": tc.full((max(self.K, 1), H * d + pad), 7.0, device="cuda")}
        p = {k: (x.data_ptr() if k in want else None) for k, x in buf.items()}
        ptr = lambda x: x.data_ptr() if x is not None else None   # noqa: E731
        self.eng.edge_dot_backward_device(H, d, ptr(Xb), H * d, ptr(Yb), H * d, Gb.data_ptr(), H + gpad, p["dX"], H * d + pad, p["dY"],
                                          H * d + pad, self.stream())
        tc.cuda.synchronize()
        out = {k: x.cpu().numpy() for k, x in buf.items()}
        out["dX"], out["dY"] = out["dX"][:self.M], out["dY"][:self.K]
        return out

    def weight_passes(self, X, Y, Gs, H, d):
        """the two score-attention passes the backward is defined by: O of the WEIGHT forward (S := Gs, V := Y), dV of the WEIGHT
        backward's column pass (S := Gs, G := X; V is not read)"""
        tc = self.t
        Xb, Yb, Gb = self.dev(X), self.dev(Y), self.dev(Gs)
        O, dV = tc.full((self.M, H * d), 7.0, device="cuda"), tc.full((self.K, H * d), 7.0, device="cuda")
        self.eng.score_attention_device(WEIGHT, H, d, Gb.data_ptr(), H, Yb.data_ptr(), H * d, O.data_ptr(), H * d, None, None, self.stream())
        self.eng.score_attention_backward_device(WEIGHT, H, d, Gb.data_ptr(), H, Yb.data_ptr(), H * d, None, H * d, None, Xb.data_ptr(), H * d, None,
                                                 H, dV.data_ptr(), H * d, None, self.stream())
        tc.cuda.synchronize()
        return O.cpu().numpy(), dV.cpu().numpy()


# --- forward bits ------------------------------------------------------------------------------------------------------------------------
_patterns = {}


def forward_patterns():
    if not _patterns:
        p = pat("P")
        _patterns["P"] = (p.rp, p.ci, p.M, p.K)
        _, rp, ci, _, M, K = base_matrix(5)
        _patterns["base"] = (rp, ci, M, K)
        _patterns.update(small_patterns())
    return _patterns


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("H", HEADS)
def test_forward_bits_numpy_loop_and_sddmm_per_head(sx, H, d):
    p = pat("P")
    assert {2046, 2048} <= set(p.lens.tolist()) and len(p.empty) > 0
    for name, (rp, ci, M, K) in forward_patterns().items():
        rs = rng("edge_dot", H, d, name)
        X, Y = rand(rs, M, H * d), rand(rs, K, H * d)
        a = DotAbi(sx, rp, ci, M, K)
        S, _ = a.fwd(X, Y, H, d)
        assert a.eng.last_kernel() == "edge_dot"
        want = dot_ref(rp, ci, X, Y, H, d)
        assert np.any(want != 0) and bits_equal(S, want), name
        assert bits_equal(S, a.sddmm(X, Y, H, d)), name
        if name in ("base", "nnz257"):
            # padded buffers: NaN beyond heads * d in X and Y is not read; lds > heads: one store per element, the padding survives
            S2, Sb = a.fwd(X, Y, H, d, pad=(4, 8, 0))
            assert same(S2, S), name
            S3, Sb = a.fwd(X, Y, H, d, pad=(8, 4, 5))
            assert same(S3, S) and np.all(Sb[:, H:] == POISON), name
        a.eng.close()


@pytest.mark.parametrize("name", ["P", "PT"])
@pytest.mark.parametrize("H, d", [(1, 8), (3, 128), (8, 16)])
def test_exact_on_integers(sx, H, d, name):
    p, other = pat(name), pat("PT" if name == "P" else "P")   # other: the pattern the pass for dY walks
    assert p.long_rows != other.long_rows
    rs = rng("edge_dot_int", H, d, name)
    X, Y, Gs = ints(rs, p.M, H * d), ints(rs, p.K, H * d), ints(rs, p.nnz, H)
    a = DotAbi(sx, p.rp, p.ci, p.M, p.K)
    S, _ = a.fwd(X, Y, H, d)
    want = dot_ref(p.rp, p.ci, X, Y, H, d, np.int64)
    assert np.abs(want).max() <= 16 * d <= 2048
    assert np.array_equal(S, want.astype(np.float32))
    got = a.bwd(X, Y, Gs, H, d)
    assert a.eng.last_kernel() == "edge_dot_backward+long_rows"   # one of the two passes walks the pattern with the long rows
    ref, mags, _ = grad_ref(p.rp, p.ci, X, Y, Gs, p.M, p.K, H, d, np.int64)
    for g in GRADS:
        assert mags[g].max() < 2 ** 24
        assert np.array_equal(got[g], ref[g].astype(np.float32)), g
    # each pass alone names the kernel of the pattern it walks
    a.bwd(X, Y, Gs, H, d, want=("dX",))
    assert a.eng.last_kernel() == "edge_dot_backward" + ("+long_rows" if p.long_rows else "")
    a.bwd(X, Y, Gs, H, d, want=("dY",))
    assert a.eng.last_kernel() == "edge_dot_backward" + ("+long_rows" if other.long_rows else "")
    # rows and columns without entries: the bits of +0
    empty_cols = np.flatnonzero(np.bincount(p.ci, minlength=p.K) == 0)
    assert len(p.empty) + len(empty_cols) == 5
    assert np.all(got["dX"][p.empty].view(np.uint32) == 0) and np.all(got["dY"][empty_cols].view(np.uint32) == 0)
    a.eng.close()


# --- backward on random real operands --------------------------------------------------------------------------------------------------
_cases = {}


def base_case(H, d):
    """the 400 x 300 matrix of the reduce tests (empty rows, one row of 300), operands uniform in +-1, once per shape"""
    if (H, d) not in _cases:
        rs, rp, ci, _, M, K = base_matrix(5)
        _cases[H, d] = (rp, ci, M, K, rand(rs, M, H * d), rand(rs, K, H * d), rand(rs, len(ci), H))
    return _cases[H, d]


@pytest.mark.parametrize("H, d", [(1, 8), (3, 24), (8, 16), (2, 64), (3, 128)])
def test_backward_bits_bound_pass_selection_and_leading_dimensions(sx, H, d):
    rp, ci, M, K, X, Y, Gs = base_case(H, d)
    a = DotAbi(sx, rp, ci, M, K)
    a.fwd(X, Y, H, d)
    alone = {"dX": a.bwd(X, Y, Gs, H, d, want=("dX",))}
    assert a.eng.get_stat("transpose_build_s") == 0   # the forward and dX alone need no A^T: none is built
    got = a.bwd(X, Y, Gs, H, d)
    assert a.eng.last_kernel() == "edge_dot_backward"
    assert a.eng.get_stat("transpose_build_s") > 0
    alone["dY"] = a.bwd(X, Y, Gs, H, d, want=("dY",))
    O, dV = a.weight_passes(X, Y, Gs, H, d)
    assert np.any(O != 0) and bits_equal(got["dX"], O)
    assert np.any(dV != 0) and bits_equal(got["dY"], dV)
    ref, mags, counts = grad_ref(rp, ci, X, Y, Gs, M, K, H, d)
    for g in GRADS:
        assert within_bound(got[g], ref[g], mags[g], counts[g], "%s H=%d d=%d" % (g, H, d)), g
        assert np.all(got[g][counts[g] == 0].view(np.uint32) == 0), g
        # each gradient alone: the same bits, the other's buffer untouched
        assert same(alone[g][g], got[g]), g
        assert np.all(alone[g][[x for x in GRADS if x != g][0]] == 7.0), g
    with pytest.raises(sx.SextansError):   # no gradient at all
        a.bwd(X, Y, Gs, H, d, want=())
    wide = a.bwd(X, Y, Gs, H, d, pad=12, gpad=3)
    for g in GRADS:
        assert same(wide[g][:, :H * d], got[g]) and np.all(wide[g][:, H * d:] == 7.0), g
    a.eng.close()


def test_special_values(sx):
    """a NaN in one X row and an inf in one Y row: they appear in that row's and that column's entries of S, in the gradient rows that
    read them, in their head and column, only"""
    H, d = 3, 24
    rp, ci, M, K, X, Y, Gs = base_case(H, d)
    rows = rows_of(rp)
    c0 = int(np.argmax(np.bincount(ci, minlength=K)))                 # the fullest column
    r0 = int(np.flatnonzero((np.diff(rp) >= 3) & (np.diff(rp) < 50))[7])   # a row of a few entries
    X2, Y2 = X.copy(), Y.copy()
    X2[r0, 0 * d + 5] = np.nan          # head 0, column 5
    Y2[c0, 2 * d + 17] = np.inf         # head 2, column 17
    a = DotAbi(sx, rp, ci, M, K)
    S, _ = a.fwd(X2, Y2, H, d)
    S0, _ = a.fwd(X, Y, H, d)
    hit = np.zeros(S.shape, bool)
    hit[rows == r0, 0] = True
    hit[ci == c0, 2] = True
    assert np.array_equal(~np.isfinite(S), hit) and same(S[~hit], S0[~hit])
    assert np.all(np.isnan(S[rows == r0, 0]))
    got, got0 = a.bwd(X2, Y2, Gs, H, d), a.bwd(X, Y, Gs, H, d)
    a.eng.close()
    hx = np.zeros((M, H * d), bool)
    hx[np.unique(rows[ci == c0]), 2 * d + 17] = True       # Y's row multiplies the terms of the rows that hold c0
    hy = np.zeros((K, H * d), bool)
    hy[np.unique(ci[rows == r0]), 0 * d + 5] = True        # X's row multiplies the terms of the columns of r0
    for g, h in (("dX", hx), ("dY", hy)):
        assert np.array_equal(~np.isfinite(got[g]), h), g
        assert same(got[g][~h], got0[g][~h]), g


def test_degenerate_matrices(sx):
    """M == 0 and nnz == 0: OK, S has no element, dX and dY are zeroed in full; K beyond every column used: those rows of dY are +0"""
    H, d = 3, 16
    rs = np.random.RandomState(4)
    for M, K in ((0, 7), (9, 7)):
        rp, ci = np.zeros(M + 1, np.int32), np.zeros(0, np.int32)
        X, Y, Gs = rand(rs, M, H * d), rand(rs, K, H * d), np.zeros((0, H), np.float32)
        a = DotAbi(sx, rp, ci, M, K)
        S, Sb = a.fwd(X, Y, H, d)
        assert S.shape == (0, H)
        got = a.bwd(X, Y, Gs, H, d, pad=4)
        for g, n in (("dX", M), ("dY", K)):
            assert got[g].shape == (n, H * d + 4) and np.all(got[g][:, :H * d].view(np.uint32) == 0) and np.all(got[g][:, H * d:] == 7.0), g
        for g in GRADS:
            alone = a.bwd(X, Y, Gs, H, d, want=(g,))
            assert np.all(alone[g].view(np.uint32) == 0) and np.all(alone[[x for x in GRADS if x != g][0]] == 7.0), g
        a.eng.close()
    # 40 rows on the first 20 of 500 columns
    M, K = 40, 500
    rp, ci, _, _ = from_lens(rs, list(rs.randint(0, 12, M)), 20)
    X, Y, Gs = rand(rs, M, H * d), rand(rs, K, H * d), rand(rs, len(ci), H)
    a = DotAbi(sx, rp, ci, M, K)
    S, _ = a.fwd(X, Y, H, d)
    assert bits_equal(S, dot_ref(rp, ci, X, Y, H, d))
    got = a.bwd(X, Y, Gs, H, d)
    ref, mags, counts = grad_ref(rp, ci, X, Y, Gs, M, K, H, d)
    for g in GRADS:
        assert within_bound(got[g], ref[g], mags[g], counts[g], g), g
    assert np.all(got["dY"][20:].view(np.uint32) == 0) and np.any(got["dY"][:20] != 0)
    a.eng.close()


def test_determinism_streams_and_graph_replay(sx):
    import torch
    H, d = 3, 24
    rp, ci, M, K, X, Y, Gs = base_case(H, d)
    a = DotAbi(sx, rp, ci, M, K)

    def both(x, y, gs):
        S, _ = a.fwd(x, y, H, d)
        g = a.bwd(x, y, gs, H, d)
        return [S, g["dX"], g["dY"]]

    first, second = both(X, Y, Gs), both(X, Y, Gs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = both(X, Y, Gs)
    torch.cuda.current_stream().wait_stream(side)
    for i, (x, y, z) in enumerate(zip(first, second, third)):
        assert same(x, y) and same(x, z), i
    rs = np.random.RandomState(77)
    X2, Y2, Gs2 = rand(rs, M, H * d), rand(rs, K, H * d), rand(rs, len(ci), H)
    other = both(X2, Y2, Gs2)
    assert not same(other[0], first[0])

    # a fresh engine: prepare() alone builds the row table, the tables of the passes and A^T, then forward and backward are captured on a
    # single stream and replayed with the operands' contents changed in place between the replays
    b = DotAbi(sx, rp, ci, M, K)
    b.eng.prepare(H * d, True, torch.cuda.current_stream().cuda_stream, transposed=True)
    torch.cuda.synchronize()
    Xt, Yt, Gt = b.dev(X), b.dev(Y), b.dev(Gs)
    St, dX, dY = torch.zeros((b.nnz, H), device="cuda"), torch.zeros((M, H * d), device="cuda"), torch.zeros((K, H * d), device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        s = torch.cuda.current_stream().cuda_stream
        b.eng.edge_dot_device(H, d, Xt.data_ptr(), H * d, Yt.data_ptr(), H * d, St.data_ptr(), H, s)
        b.eng.edge_dot_backward_device(H, d, Xt.data_ptr(), H * d, Yt.data_ptr(), H * d, Gt.data_ptr(), H, dX.data_ptr(), H * d, dY.data_ptr(),
                                       H * d, s)
    for operands, want in (((X, Y, Gs), first), ((X2, Y2, Gs2), other), ((X, Y, Gs), first)):
        for t, x in zip((Xt, Yt, Gt), operands):
            t.copy_(torch.from_numpy(x))
        for t in (St, dX, dY):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for i, (x, y) in enumerate(zip((St, dX, dY), want)):
            assert same(x.cpu().numpy(), y), i
    a.eng.close()
    b.eng.close()
