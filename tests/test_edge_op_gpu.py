"""Edge-output ops from both endpoints on the GPU through the C ABI (sextans_edge_op_device_rm / _backward_device_rm).
  Dealing: the 92-row pattern P of test_pattern_dealing_gpu.py (second walk, long-row kernel, the 2046 / 2048-entry boundary rows, empty
rows) and its transpose, at every slot width of the family plus N = 136 (a full tile and a tile of 8), all five ops with and without E,
on integer operands in [-4, 4]: every term is an integer of magnitude at most 16 and every partial sum of at most 2600 of them an exact
integer below 2^24 in any order, so Z, dx_dst and dx_src must EQUAL the int64 computation.
  Random real operands on the 400 x 300 matrix of the reduce tests: Z has the bits of the numpy float32 expression, MUL those of
sextans_spmm_edge_backward_device_rm's dE (G := x_dst, B := x_src), ADD with E those of sextans_spmm_gated_device_rm's z; the gradients
lie within (n + 2) 2^-24 sum |t_e| of a float64 reference, n the entries of the row or column -- the bound of an fp32 sum of n terms in
any order ((n - 1) 2^-24 sum |t_e| to first order, rounded up to n + 1 for the higher-order terms) plus one 2^-24 |t_e| for the rounding
of each product (MUL's fmaf rounds once, so this is generous there).  It is derived, not measured.
  Pass selection, leading dimensions, special values, degenerate matrices, determinism across runs, streams and a replayed graph."""
import numpy as np
import pytest

import test_spmm_edge_gpu as sedge
import test_spmm_gated_gpu as gated
from test_fused_attention_gpu import rand, same
from test_pattern_dealing_gpu import TILED, pat, rng
from test_spmm_edge_gpu import ints, rows_of
from test_spmm_reduce_gpu import POISON, Abi, base_matrix, bits_equal

pytestmark = pytest.mark.gpu

OPS = {"add": 1, "sub": 2, "mul": 3, "dst": 4, "src": 5}   # SEXTANS_EDGEOP_*
GRADS = ("dxdst", "dxsrc")
SIZES = [8, 24, 72, 200]   # one tile; a partial tile; two tiles of 64 the last one partial; a tile of 128 and a partial one
EPS = 2.0 ** -24


def grads_of(op):
    return [g for g in GRADS if not (op == "src" and g == "dxdst") and not (op == "dst" and g == "dxsrc")]


def forward_ref(op, rp, ci, xd, xs, E, dtype=np.float32):
    """(nnz, N) in `dtype`: one operation per element, and a second one with E"""
    d, s = xd.astype(dtype)[rows_of(rp)], xs.astype(dtype)[ci]
    z = d + s if op == "add" else d - s if op == "sub" else d * s if op == "mul" else d if op == "dst" else s
    if E is not None:
        z = z + E.astype(dtype)
    assert z.dtype == dtype
    return z


def backward_ref(op, rp, ci, xd, xs, Gz, M, K, dtype=np.float64):
    """-> {dxdst, dxsrc} (None where the op has none) in `dtype`, {the sums of |t_e|}, {the entry counts}"""
    rows = rows_of(rp)
    g = Gz.astype(dtype)
    td = g * xs.astype(dtype)[ci] if op == "mul" else g
    ts = g * xd.astype(dtype)[rows] if op == "mul" else -g if op == "sub" else g
    out, mags = {}, {}
    for name, idx, t, n in (("dxdst", rows, td, M), ("dxsrc", ci, ts, K)):
        if name not in grads_of(op):
            out[name] = mags[name] = None
            continue
        out[name], mags[name] = np.zeros((n, g.shape[1]), dtype), np.zeros((n, g.shape[1]), dtype)
        np.add.at(out[name], idx, t)
        np.add.at(mags[name], idx, np.abs(t))
    counts = {"dxdst": np.diff(rp), "dxsrc": np.bincount(ci, minlength=K)}
    return out, mags, counts


def within_bound(got, want, mags, counts, what=""):
    bound = (counts[:, None] + 2) * EPS * mags
    err = np.abs(got.astype(np.float64) - want)
    pos = bound > 0
    print(what, "max |got - want|", float(err.max()) if err.size else 0.0, "max err / bound",
          float((err[pos] / bound[pos]).max()) if np.any(pos) else 0.0)
    return bool(np.all(err <= bound))


class EdgeOpAbi(Abi):
    """test_spmm_reduce_gpu.Abi's engine on a pattern (values 1: never read), the edge op's entry points called through api.Engine"""

    def __init__(self, sx, rp, ci, M, K):
        super().__init__(sx, rp, ci, np.ones(len(ci), np.float32), M, K)

    def dev(self, x, pad=0):
        """a numpy (rows, N) operand in a device buffer `pad` columns wider (NaN there), or None"""
        if x is None:
            return None
        tc = self.t
        buf = tc.full((max(x.shape[0], 1), x.shape[1] + pad), float("nan"), device="cuda")
        buf[:x.shape[0], :x.shape[1]] = tc.from_numpy(np.ascontiguousarray(x))
        return buf

    def fwd(self, op, xd, xs, E, N=None, pad=(0, 0, 0, 0)):
        """-> Z as numpy float32 and the whole padded buffer as int32; pad: extra columns of the xdst / xsrc / E / Z buffers.  The
        operand the op does not read may be None."""
        tc = self.t
        N = N or (xd if xd is not None else xs).shape[1]
        db, sb, Eb = self.dev(xd, pad[0]), self.dev(xs, pad[1]), self.dev(E, pad[2])
        Zb = tc.full((max(self.nnz, 1), N + pad[3]), POISON, dtype=tc.int32, device="cuda")
        ptr = lambda x: x.data_ptr() if x is not None else None   # noqa: E731
        self.eng.edge_op_device_rm(OPS[op], N, ptr(db), N + pad[0], ptr(sb), N + pad[1], ptr(Eb), N + pad[2], Zb.data_ptr(), N + pad[3],
                                   tc.cuda.current_stream().cuda_stream)
        tc.cuda.synchronize()
        Zn = Zb.cpu().numpy()[:self.nnz]
        return Zn[:, :N].view(np.float32), Zn

    def bwd(self, op, xd, xs, Gz, want=GRADS, pad=0):
        """-> {name: numpy} of both gradients, each in a buffer `pad` columns wider that held 7.0: the one not in `want` gets no pointer
        and must keep its 7.0"""
        tc = self.t
        N = Gz.shape[1]
        db, sb, Gb = self.dev(xd), self.dev(xs), self.dev(Gz)
        buf = {"dxdst": tc.full((max(self.M, 1), N + pad), 7.0, device="cuda"), "dxsrc": tc.full((max(self.K, 1), N + pad), 7.0, device="cuda")}
        p = {k: (x.data_ptr() if k in want else None) for k, x in buf.items()}
        ptr = lambda x: x.data_ptr() if x is not None else None   # noqa: E731
        self.eng.edge_op_backward_device_rm(OPS[op], N, ptr(db), N, ptr(sb), N, ptr(Gb), N, p["dxdst"], N + pad, p["dxsrc"], N + pad,
                                            tc.cuda.current_stream().cuda_stream)
        tc.cuda.synchronize()
        out = {k: x.cpu().numpy() for k, x in buf.items()}
        out["dxdst"], out["dxsrc"] = out["dxdst"][:self.M], out["dxsrc"][:self.K]
        return out


# --- dealing: every path, every width, exact integers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["P", "PT"])
@pytest.mark.parametrize("N", TILED)
def test_every_dealing_path_exact_on_integers(sx, N, name):
    p, other = pat(name), pat("PT" if name == "P" else "P")   # other: the pattern the pass for dx_src walks
    assert p.long_rows != other.long_rows
    rs = rng("edge_op", N, name)
    xd, xs, E, Gz = ints(rs, p.M, N), ints(rs, p.K, N), ints(rs, p.nnz, N), ints(rs, p.nnz, N)
    empty_cols = np.flatnonzero(np.bincount(p.ci, minlength=p.K) == 0)
    assert len(p.empty) + len(empty_cols) == 5
    a = EdgeOpAbi(sx, p.rp, p.ci, p.M, p.K)
    for op in OPS:
        for e in (None, E):
            Z, _ = a.fwd(op, xd, xs, e)
            assert a.eng.last_kernel() == "edge_op" + ("+long_rows" if p.long_rows else ""), (op, a.eng.last_kernel())
            want = forward_ref(op, p.rp, p.ci, xd, xs, e, np.int64)
            assert np.array_equal(Z, want.astype(np.float32)), (op, e is not None)
        names = grads_of(op)
        got = a.bwd(op, xd, xs, Gz, want=names)
        long = ("dxdst" in names and p.long_rows) or ("dxsrc" in names and other.long_rows)
        assert a.eng.last_kernel() == "edge_op_backward" + ("+long_rows" if long else ""), (op, a.eng.last_kernel())
        want, _, _ = backward_ref(op, p.rp, p.ci, xd, xs, Gz, p.M, p.K, np.int64)
        for g in names:
            assert np.array_equal(got[g], want[g].astype(np.float32)), (op, g)
        # each pass alone names the kernel of the pattern it walks
        if len(names) == 2:
            a.bwd(op, xd, xs, Gz, want=("dxdst",))
            assert a.eng.last_kernel() == "edge_op_backward" + ("+long_rows" if p.long_rows else "")
            a.bwd(op, xd, xs, Gz, want=("dxsrc",))
            assert a.eng.last_kernel() == "edge_op_backward" + ("+long_rows" if other.long_rows else "")
        # rows and columns without entries: the bits of +0
        if "dxdst" in names:
            assert np.all(got["dxdst"][p.empty].view(np.uint32) == 0), op
        if "dxsrc" in names:
            assert np.all(got["dxsrc"][empty_cols].view(np.uint32) == 0), op
    a.eng.close()


# --- random real operands ----------------------------------------------------------------------------------------------------------------
_cases = {}


def base_case(N):
    """the 400 x 300 matrix of the reduce tests (empty rows, one row of 300), operands uniform in +-1, once per N"""
    if N not in _cases:
        rs, rp, ci, _, M, K = base_matrix(5)
        nnz = len(ci)
        _cases[N] = (rp, ci, M, K, rand(rs, M, N), rand(rs, K, N), rand(rs, nnz, N), rand(rs, nnz, N))
    return _cases[N]


@pytest.mark.parametrize("N", SIZES)
def test_random_operands_bits_bound_pass_selection_and_leading_dimensions(sx, N):
    rp, ci, M, K, xd, xs, E, Gz = base_case(N)
    nnz = len(ci)
    assert 200 <= M <= 999 and 2000 <= nnz <= 9999
    a = EdgeOpAbi(sx, rp, ci, M, K)
    Zs = {}
    for op in OPS:
        for e in (None, E):
            Z, _ = a.fwd(op, xd, xs, e)
            assert a.eng.last_kernel() == "edge_op"
            assert bits_equal(Z, forward_ref(op, rp, ci, xd, xs, e)), (op, e is not None)
            Zs[op, e is not None] = Z
        # the operand the op does not read is ignored: absent, the same bits
        if op in ("dst", "src"):
            Z2, _ = a.fwd(op, xd if op == "dst" else None, xs if op == "src" else None, E, N=N)
            assert same(Z2, Zs[op, True])
        # leading dimensions beyond N: the same bits written in place, the columns beyond N left alone
        Z2, Zb = a.fwd(op, xd, xs, E, pad=(4, 8, 12, 16))
        assert same(Z2, Zs[op, True]) and np.all(Zb[:, N:] == POISON)
        names = grads_of(op)
        alone = {g: a.bwd(op, xd, xs, Gz, want=(g,)) for g in names if g != "dxsrc"}
        if op == "add":   # (the first op) the forward and dx_dst alone need no A^T: none is built
            assert a.eng.get_stat("transpose_build_s") == 0
        got = a.bwd(op, xd, xs, Gz, want=names)
        assert a.eng.last_kernel() == "edge_op_backward"
        if "dxsrc" in names:
            assert a.eng.get_stat("transpose_build_s") > 0
            alone["dxsrc"] = a.bwd(op, xd, xs, Gz, want=("dxsrc",))
        want, mags, counts = backward_ref(op, rp, ci, xd, xs, Gz, M, K)
        for g in names:
            assert within_bound(got[g], want[g], mags[g], counts[g], "%s %s N=%d" % (op, g, N)), (op, g)
            assert np.all(got[g][counts[g] == 0].view(np.uint32) == 0), (op, g)
            # each gradient alone: the same bits, the other's buffer untouched
            assert same(alone[g][g], got[g]), (op, g)
            assert np.all(alone[g][[x for x in GRADS if x != g][0]] == 7.0), (op, g)
        for g in GRADS:
            if g not in names:
                assert np.all(got[g] == 7.0)
                with pytest.raises(sx.SextansError):   # a gradient of an operand the op does not read
                    a.bwd(op, xd, xs, Gz, want=GRADS)
        with pytest.raises(sx.SextansError):           # no gradient at all
            a.bwd(op, xd, xs, Gz, want=())
        wide = a.bwd(op, xd, xs, Gz, want=names, pad=12)
        for g in names:
            assert same(wide[g][:, :N], got[g]) and np.all(wide[g][:, N:] == 7.0), (op, g)
    # SUB's dx_src: ADD's bits negated, a zero sum +0
    add, sub = a.bwd("add", xd, xs, Gz, want=("dxsrc",))["dxsrc"], a.bwd("sub", xd, xs, Gz, want=("dxsrc",))["dxsrc"]
    assert same(sub, np.where(add == 0, np.float32(0), -add))
    a.eng.close()
    # MUL: the bits of spmm_edge's dE with G := x_dst, B := x_src
    b = sedge.Abi(sx, rp, ci, M, K)
    _, dE, _, _ = b.backward("mul", xs, E, xd, want_dB=False)
    b.eng.close()
    assert np.any(dE != 0) and bits_equal(Zs["mul", False], dE)
    # ADD with E: the bits of spmm_gated's z on the same operands
    c = gated.GatedAbi(sx, rp, ci, M, K)
    z = c.fwd(gated.SUM, xd, xs, xs, E, want=("C", "z"))["z"]
    c.eng.close()
    assert np.any(z != 0) and bits_equal(Zs["add", True], z)


@pytest.mark.parametrize("op", list(OPS))
def test_special_values(sx, op):
    """a NaN and an inf in one x_src row and in one Gz entry: they appear in that column's entries, and in the rows and columns that hold
    them, only"""
    N = 24
    rp, ci, M, K, xd, xs, E, Gz = base_case(N)
    rows = rows_of(rp)
    c0 = int(np.argmax(np.bincount(ci, minlength=K)))     # the fullest column
    e0 = int(np.flatnonzero(ci != c0)[len(ci) // 2])      # an entry outside it
    xs2, Gz2 = xs.copy(), Gz.copy()
    xs2[c0, 3], xs2[c0, 17] = np.nan, np.inf
    Gz2[e0, 5], Gz2[e0, 11] = np.nan, -np.inf
    a = EdgeOpAbi(sx, rp, ci, M, K)
    Z, _ = a.fwd(op, xd, xs2, E)
    Z0, _ = a.fwd(op, xd, xs, E)
    hit = np.zeros(Z.shape, bool)
    if op != "dst":
        hit[np.ix_(ci == c0, [3, 17])] = True
    assert np.array_equal(~np.isfinite(Z), hit) and same(Z[~hit], Z0[~hit])
    names = grads_of(op)
    got, got0 = a.bwd(op, xd, xs2, Gz2, want=names), a.bwd(op, xd, xs, Gz, want=names)
    a.eng.close()
    for g in names:
        n = M if g == "dxdst" else K
        hit = np.zeros((n, N), bool)
        hit[rows[e0] if g == "dxdst" else ci[e0], [5, 11]] = True      # Gz's entry: its row, its column
        if op == "mul" and g == "dxdst":                                # x_src's row multiplies the terms of the rows that hold c0
            hit[np.ix_(np.unique(rows[ci == c0]), [3, 17])] = True
        assert np.array_equal(~np.isfinite(got[g]), hit), (op, g)
        assert same(got[g][~hit], got0[g][~hit]), (op, g)


def test_degenerate_matrices(sx):
    """M == 0 and nnz == 0: OK, Z has no element, dx_dst and dx_src are zeroed; rows of one entry: the term's own bits"""
    N = 16
    rs = np.random.RandomState(4)
    for M, K in ((0, 7), (9, 7)):
        rp, ci = np.zeros(M + 1, np.int32), np.zeros(0, np.int32)
        xd, xs, E = rand(rs, M, N), rand(rs, K, N), np.zeros((0, N), np.float32)
        a = EdgeOpAbi(sx, rp, ci, M, K)
        for op in OPS:
            Z, Zb = a.fwd(op, xd, xs, E)
            assert Z.shape == (0, N)
            got = a.bwd(op, xd, xs, E, want=grads_of(op))
            for g in grads_of(op):
                assert got[g].shape == ((M if g == "dxdst" else K), N) and np.all(got[g].view(np.uint32) == 0), (op, g)
        a.eng.close()
    # every row holds one entry: dx_dst is the term itself
    M, K = 37, 11
    rp, ci = np.arange(M + 1, dtype=np.int32), rs.randint(0, K, M).astype(np.int32)
    xd, xs, Gz = rand(rs, M, N), rand(rs, K, N), rand(rs, M, N)
    a = EdgeOpAbi(sx, rp, ci, M, K)
    for op in OPS:
        Z, _ = a.fwd(op, xd, xs, None)
        assert bits_equal(Z, forward_ref(op, rp, ci, xd, xs, None))
        if op != "src":
            got = a.bwd(op, xd, xs, Gz, want=("dxdst",))["dxdst"]
            assert bits_equal(got, (Gz * xs[ci] if op == "mul" else Gz) + np.float32(0)), op
    a.eng.close()


def test_determinism_streams_and_graph_replay(sx):
    import torch
    N, op = 24, "mul"
    rp, ci, M, K, xd, xs, E, Gz = base_case(N)
    a = EdgeOpAbi(sx, rp, ci, M, K)

    def both():
        Z, _ = a.fwd(op, xd, xs, E)
        g = a.bwd(op, xd, xs, Gz)
        return [Z, g["dxdst"], g["dxsrc"]]

    first, second = both(), both()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = both()
    torch.cuda.current_stream().wait_stream(side)
    for i, (x, y, z) in enumerate(zip(first, second, third)):
        assert same(x, y) and same(x, z), i

    # a fresh engine: prepare() alone builds the tables and A^T, then forward and backward are captured on a single stream and replayed twice
    b = EdgeOpAbi(sx, rp, ci, M, K)
    b.eng.prepare(N, True, torch.cuda.current_stream().cuda_stream, transposed=True)
    torch.cuda.synchronize()
    dt, st, Et, Gt = b.dev(xd), b.dev(xs), b.dev(E), b.dev(Gz)
    Zt, dd, ds = torch.zeros((b.nnz, N), device="cuda"), torch.zeros((M, N), device="cuda"), torch.zeros((K, N), device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        s = torch.cuda.current_stream().cuda_stream
        b.eng.edge_op_device_rm(OPS[op], N, dt.data_ptr(), N, st.data_ptr(), N, Et.data_ptr(), N, Zt.data_ptr(), N, s)
        b.eng.edge_op_backward_device_rm(OPS[op], N, dt.data_ptr(), N, st.data_ptr(), N, Gt.data_ptr(), N, dd.data_ptr(), N, ds.data_ptr(), N, s)
    for _ in range(2):
        for t in (Zt, dd, ds):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for i, (x, y) in enumerate(zip((Zt, dd, ds), first)):
            assert same(x.cpu().numpy(), y), i
    a.eng.close()
    b.eng.close()
