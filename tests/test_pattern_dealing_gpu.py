"""The row-dealing layer under every pattern pass (pattern_pass.h: pattern_rows<Pass> / pattern_long<Pass>), exercised through every
family at every slot width: fused attention, attention with edge features, GAT, GATv2, score attention, max / min reduce,
multi-aggregation, softmax aggregation and edge SpMM.
  One 92-row pattern P (dealing_pattern) puts rows on every path of the engine at once: one slot group per row (E = 1), several slots per
row (1 < E < S, E = S), a range with an idle slot group, rows for the second walk at range index < 64 and >= 64, a long row alone in its
wavefront's range, a long row that shares its range, a row that is long only through the alignment of its start (2046 entries from
b % 4 == 3) and a row of exactly 2048 aligned entries that is not long, and empty rows.  dealing() restates the dealing on the CPU and
test_the_pattern_reaches_every_path asserts that P reaches all of that for every slot count and head count (no GPU needed).
  Every GPU case runs one family at one width on P or on P^T (2600 x 92; its rows are short, its backward's column pass walks P with
P's own tables) against the family's own float64 reference under the family's own check.  The names of the kernels are asserted too:
every pass over P runs the long-row kernel ("+long_rows": the forward and backward on P, the backward on P^T); the forward on P^T does
not, P^T has no row beyond 92 entries.
  A second, sharper forward check: with all scores equal and integer values every coefficient is exactly 1 / n and every partial sum an
integer below 2^24, so O = sum / n up to the rounding of one reciprocal and one multiply -- a lost, doubled or misplaced entry moves the
sum by at least one part in 10 000.
  The dense float64 references have no answer for an empty row: they are given the pattern without its empty rows (no entry and no column
gradient changes), and what the families document for an empty row is asserted on its own."""
import bisect
import zlib

import numpy as np
import pytest

import test_attention_dropout_gpu as drp
import test_attention_edge_gpu as aedge
import test_fused_attention_gpu as att
import test_gat_attention_gpu as gat
import test_gatv2_attention_gpu as gatv2
import test_score_attention_gpu as score
import test_spmm_edge_gpu as sedge
import test_spmm_multi_gpu as multi
import test_spmm_reduce_gpu as red
import test_spmm_softagg_gpu as sagg
from test_fused_attention_gpu import rand, same
from test_gatv2_attention_gpu import grid
from test_torch_attention_gpu import make_A
from test_torch_autograd_gpu import _close

gpu = pytest.mark.gpu

LENS = [1] * 30 + [40] + [1] * 40 + [150] + [252] + [100, 100, 56] + [10] * 5 + [1] + [2046] + [3] + [2048] + [2500] + [0, 0, 0] + [5] + [0, 0]
COLS = 2600
CHUNK = 2048           # kSoftmaxChunk
WAVE_ENTRIES = 256     # kSoftmaxWaveEntries
WIDTHS = [8, 16, 32, 64, 128]
TILED = [8, 16, 32, 64, 128, 136]   # the tiled families' N: 136 is a tile of 128 and one of 8
HEADS = [1, 3]
PATTERNS = ["P", "PT"]
SLOPE, SCALE = 0.2, 0.37


# --- the input -------------------------------------------------------------------------------------------------------------------------
def dealing_pattern(rs):
    """-> rp, ci, M, K: rows of LENS entries, each row's columns sorted and distinct"""
    M = len(LENS)
    rp = np.zeros(M + 1, np.int32); rp[1:] = np.cumsum(LENS)
    ci = np.zeros(rp[-1], np.int32)
    for r, n in enumerate(LENS):
        ci[rp[r]:rp[r + 1]] = np.sort(rs.choice(COLS, n, replace=False))
    return rp, ci, M, COLS


def transposed(rp, ci, M, K):
    """the pattern of the transpose, built on the host: -> rp, ci, K, M (a stable sort keeps every row's columns ascending)"""
    rows = np.repeat(np.arange(M, dtype=np.int32), np.diff(rp))
    order = np.argsort(ci, kind="stable")
    rpt = np.zeros(K + 1, np.int32); rpt[1:] = np.cumsum(np.bincount(ci, minlength=K))
    return rpt, rows[order].astype(np.int32), K, M


class Pat:
    def __init__(self, rp, ci, M, K):
        self.rp, self.ci, self.M, self.K, self.nnz = rp, ci, M, K, len(ci)
        self.lens = np.diff(rp)
        self.ne, self.empty = np.flatnonzero(self.lens > 0), np.flatnonzero(self.lens == 0)
        self.rp_ne = np.zeros(len(self.ne) + 1, np.int32); self.rp_ne[1:] = np.cumsum(self.lens[self.ne])   # without the empty rows
        self.long_rows = bool(np.any(long_rows_of(rp)))


_pats = {}


def pat(name):
    if not _pats:
        rp, ci, M, K = dealing_pattern(np.random.RandomState(92))
        _pats["P"], _pats["PT"] = Pat(rp, ci, M, K), Pat(*transposed(rp, ci, M, K))
    return _pats[name]


def rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


# --- the CPU model ---------------------------------------------------------------------------------------------------------------------
def row_span(b, e):
    return e - (b & ~3)


def long_rows_of(rp):
    """what softmax_count_long / softmax_fill_long put in the long-row table"""
    return np.array([rp[r + 1] > rp[r] and row_span(int(rp[r]), int(rp[r + 1])) > CHUNK for r in range(len(rp) - 1)], bool)


def dealing(rp, S, HS):
    """The row-dealing part of attn_rows_body for a wavefront of S slots that deals HS heads per row (HS = 1: heads_inside, or one
    head) -> one dict per non-empty range: w, ra, rb, E, cap, idle (some slot group has no item in the last round) and path[r - ra] in
    "group" (walked by its slot group; an empty row is one without entries), "big" (the second walk) or "long" (pattern_long).
    THIS RESTATES pattern_pass.h (and softmax_wave_rows of row_softmax_kernels.h) AND MUST MOVE WITH THEM."""
    rp = [int(x) for x in rp]
    M, nnz = len(rp) - 1, rp[-1]
    nw = -(-nnz // WAVE_ENTRIES)
    wrow = [bisect.bisect_left(rp, WAVE_ENTRIES * w, 0, M) for w in range(nw)] + [M]
    out = []
    for w in range(nw):
        ra, rb = wrow[w], wrow[w + 1]
        if ra >= rb:
            continue
        total, rows = rp[rb] - rp[ra], rb - ra
        if row_span(rp[rb - 1], rp[rb]) > CHUNK and rows > 1:   # a long row is the last of its range and does not count
            total -= rp[rb] - rp[rb - 1]
            rows -= 1
        items = (rb - ra) * HS
        E = 1
        while 2 * E <= S and 2 * E * items <= S:
            E *= 2
        cap = float("inf") if E == S else E * max(32, 4 * (total // rows))
        path = []
        for r in range(ra, rb):
            b, e = rp[r], rp[r + 1]
            path.append("long" if e > b and row_span(b, e) > CHUNK else "big" if e - b > cap else "group")
        out.append(dict(w=w, ra=ra, rb=rb, E=E, cap=cap, idle=items % (S // E) != 0, path=path))
    return out


@pytest.mark.parametrize("HS", [1, 2, 3])
@pytest.mark.parametrize("S", [32, 16, 8])
def test_the_pattern_reaches_every_path(S, HS):
    p = pat("P")
    rp, lens = p.rp, p.lens
    assert p.M == 92 and p.nnz == 7421 and p.K == 2600
    assert all(np.all(np.diff(p.ci[rp[r]:rp[r + 1]]) > 0) for r in range(p.M)) and p.ci.max() < p.K
    ranges = dealing(rp, S, HS)
    byw = {g["w"]: g for g in ranges}
    assert sorted(byw) == [0, 1, 2, 3, 11, 19, 28], sorted(byw)
    assert [byw[w]["rb"] - byw[w]["ra"] for w in (0, 1, 2, 3, 11, 19, 28)] == [72, 1, 3, 7, 2, 1, 6]
    assert any(g["E"] == 1 for g in ranges)
    assert any(1 < g["E"] < S for g in ranges)
    assert any(g["idle"] for g in ranges)
    if (S, HS) != (8, 2):   # ... and one whose idle lanes take part in a merge's shuffles (8 slots, 2 heads: every E > 1 range is full)
        assert any(g["idle"] and g["E"] > 1 for g in ranges)
    big = [(g, i) for g in ranges for i, x in enumerate(g["path"]) if x == "big"]
    assert any(i < 64 for _, i in big) and any(i >= 64 for _, i in big)
    assert [(i, int(lens[byw[0]["ra"] + i])) for g, i in big if g["w"] == 0] == [(30, 40), (71, 150)]
    longs = [(g, g["ra"] + i) for g in ranges for i, x in enumerate(g["path"]) if x == "long"]
    assert sorted(int(lens[r]) for _, r in longs) == [2046, 2500]
    assert np.array_equal(np.flatnonzero(long_rows_of(rp)), sorted(r for _, r in longs))     # the table and the kernels agree
    assert any(g["rb"] - g["ra"] == 1 for g, _ in longs)                                     # a long row alone in its range
    assert any(g["rb"] - g["ra"] > 1 and r == g["rb"] - 1 for g, r in longs)                 # one that shares it (and is its last row)
    assert any(lens[r] <= CHUNK for _, r in longs)                                           # long through its start's alignment
    r2046, r2048 = int(np.flatnonzero(lens == 2046)[0]), int(np.flatnonzero(lens == 2048)[0])
    assert rp[r2046] % 4 == 3 and row_span(int(rp[r2046]), int(rp[r2046 + 1])) == 2049
    assert rp[r2048] % 4 == 0 and row_span(int(rp[r2048]), int(rp[r2048 + 1])) == 2048
    g = byw[11]
    assert g["path"][r2048 - g["ra"]] in ("group", "big")                                    # 2048 entries, finished in pattern_rows
    assert any(lens[g["ra"] + i] == 0 for g in ranges for i, x in enumerate(g["path"]) if x == "group")
    if HS == 1:
        assert any(g["E"] == S for g in ranges)
    # P^T: no long row of its own (its forward runs pattern_rows alone), a table of its own
    t = pat("PT")
    assert t.M == 2600 and t.K == 92 and t.nnz == p.nnz and t.lens.max() <= 92 and not t.long_rows and p.long_rows
    assert len(p.empty) == 5   # (every column of P holds an entry: P^T has no empty row)


# --- what the cases share --------------------------------------------------------------------------------------------------------------
def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(*xs):
    return [x.cpu().numpy() if x is not None else None for x in xs]


def names_ok(p, base, fwd, bwd, dropout=False):
    """every pass over P runs the long-row kernel: the forward on P, the backward on P and on P^T (its column pass)"""
    mid = "+dropout" if dropout else ""
    assert fwd == base + mid + ("+long_rows" if p.long_rows else ""), fwd
    if bwd is not None:
        assert bwd == base + "_backward" + mid + "+long_rows", bwd


def empty_rows_ok(p, O, lse=None, zero=()):
    """what every family documents for a row without entries (P has five): O = +0 (the bits), lse = -inf, zero gradients"""
    assert np.all(np.ascontiguousarray(O[p.empty]).view(np.uint32) == 0)
    if lse is not None:
        assert np.all(lse[p.empty] == -np.inf)
    for g in zero:
        assert np.all(g[p.empty] == 0)


def gat_scores(rs, M, K, H):
    """a_dst, a_src on GATv2's grid: z = (i + j + 1/2) / 32 stays 1 / 64 away from LeakyReLU's kink"""
    return grid(rs, M, H, 1, False)[:, :, 0].copy(), grid(rs, K, H, 1, True)[:, :, 0].copy()


def int_values(rs, *shape):
    """integers from {+-1 .. +-4}, never 0"""
    return (rs.randint(1, 5, shape) * rs.choice([-1, 1], shape)).astype(np.float32)


cases = lambda f: pytest.mark.parametrize("name", PATTERNS)(pytest.mark.parametrize("H", HEADS)(pytest.mark.parametrize("w", WIDTHS)(gpu(f))))   # noqa: E731
tiled_cases = lambda f: pytest.mark.parametrize("name", PATTERNS)(pytest.mark.parametrize("N", TILED)(gpu(f)))   # noqa: E731


# --- 3. family x width x heads x {P, P^T}: forward and backward against float64 ------------------------------------------------------------
@pytest.mark.parametrize("bias", [False, True])
@cases
def test_fused_attention(sx, w, H, name, bias):
    """bias with dbias requested: the row pass takes all heads of a row inside one slot group (heads_inside)"""
    p, rs = pat(name), rng("attention", w, H, name, bias)
    M, K = p.M, p.K
    v = rand(rs, p.nnz)
    Qn, Kn, Vn, Gn = rand(rs, M, H, w), rand(rs, K, H, w), rand(rs, K, H, w), rand(rs, M, H, w)
    Q, Kt, V, G = (dev(x) for x in (Qn, Kn, Vn, Gn))
    b = dev(v) if bias else None
    a = att.Abi(sx, p.rp, p.ci, M, K, H, w, w)
    O, lse = a.forward(Q, Kt, V, b, SCALE)
    fwd = a.eng.last_kernel()
    dQ, dK, dV, db = a.backward(Q, Kt, V, b, SCALE, O, lse, G, want_dbias=bias)
    names_ok(p, "attention_fused", fwd, a.eng.last_kernel())
    O, lse, dQ, dK, dV, db = host(O, lse, dQ, dK, dV, db)
    a.eng.close()
    ne = p.ne
    want = att.reference(p.rp_ne, p.ci, v, len(ne), K, Qn[ne], Kn, Vn, Gn[ne], SCALE, bias)
    att.check([O[ne], dQ[ne], dK, dV, db], want, bias)
    assert np.all(np.isfinite(lse[ne]))
    empty_rows_ok(p, O, lse, zero=(dQ,))


@cases
def test_attention_edge(sx, w, H, name):
    p, rs = pat(name), rng("attention_edge", w, H, name)
    ops, G = aedge.operands(rs, p.M, p.K, p.nnz, H, w, w, "both", True)
    a = aedge.Abi(sx, p.rp, p.ci, p.M, p.K, H, w, w)
    got = a.run(ops, G, SCALE)
    names_ok(p, "attention_edge_fused", a.fwd_kernel, a.eng.last_kernel())
    a.eng.close()
    aedge.check(got, aedge.reference(p.rp, p.ci, p.M, ops, G, SCALE))
    empty_rows_ok(p, got["O"], got["lse"], zero=(got["dQ"],))


@cases
def test_gat(sx, w, H, name):
    p, rs = pat(name), rng("gat", w, H, name)
    M, K = p.M, p.K
    adn, asn = gat_scores(rs, M, K, H)
    Vn, Gn = rand(rs, K, H, w), rand(rs, M, H, w)
    gat.assert_off_the_kink(p.rp, p.ci, adn, asn)
    ad, as_, V, G = (dev(x) for x in (adn, asn, Vn, Gn))
    a = gat.Abi(sx, p.rp, p.ci, M, K, H, w)
    O, lse = a.forward(ad, as_, V, None, SLOPE)
    fwd = a.eng.last_kernel()
    dad, das, dV, _ = a.backward(ad, as_, V, None, SLOPE, O, lse, G, want_dbias=False)
    names_ok(p, "gat_fused", fwd, a.eng.last_kernel())
    O, lse, dad, das, dV = host(O, lse, dad, das, dV)
    a.eng.close()
    ne = p.ne
    want = gat.reference(p.rp_ne, p.ci, np.zeros(p.nnz, np.float32), len(ne), K, adn[ne], asn, Vn, Gn[ne], SLOPE, False)
    gat.check([O[ne], dad[ne], das, dV, None], want, False)
    assert np.all(np.isfinite(lse[ne]))
    empty_rows_ok(p, O, lse, zero=(dad,))


@cases
def test_gatv2(sx, w, H, name):
    p, rs = pat(name), rng("gatv2", w, H, name)
    M, K = p.M, p.K
    xdn, xsn, attn, Gn = grid(rs, M, H, w, False), grid(rs, K, H, w, True), rand(rs, H, w), rand(rs, M, H, w)
    gatv2.assert_off_the_kink(p.rp, p.ci, xdn, xsn)
    xd, xs, at, G = (dev(x) for x in (xdn, xsn, attn, Gn))
    a = gatv2.Abi(sx, p.rp, p.ci, M, K, H, w)
    O, lse = a.forward(xd, xs, at, None, SLOPE)
    fwd = a.eng.last_kernel()
    dxd, dxs, datt, _ = a.backward(xd, xs, at, None, SLOPE, O, lse, G, want_dbias=False)
    names_ok(p, "gatv2_fused", fwd, a.eng.last_kernel())
    O, lse, dxd, dxs, datt = host(O, lse, dxd, dxs, datt)
    a.eng.close()
    gatv2.check([O, dxd, dxs, datt, None], gatv2.reference(p.rp, p.ci, M, K, xdn, xsn, attn, Gn, SLOPE), False)
    assert np.all(np.isfinite(lse[p.ne]))
    empty_rows_ok(p, O, lse, zero=(dxd,))


@pytest.mark.parametrize("mode", [score.SOFTMAX, score.WEIGHT], ids=["softmax", "weight"])
@cases
def test_score_attention(sx, w, H, name, mode):
    p, rs = pat(name), rng("score", w, H, name, mode)
    M, K = p.M, p.K
    Sn, Vn, Gn = score.scores(rs, p.nnz, H, mode), rand(rs, K, H, w), rand(rs, M, H, w)
    S, V, G = (dev(x) for x in (Sn, Vn, Gn))
    a = score.Abi(sx, p.rp, p.ci, M, K, H, w)
    O, lse = a.forward(mode, S, V)
    fwd = a.eng.last_kernel()
    dS, dV = a.backward(mode, S, V, O, lse, G)
    names_ok(p, "score_softmax_fused" if mode == score.SOFTMAX else "score_weight_fused", fwd, a.eng.last_kernel())
    O, lse, dS, dV = host(O, lse, dS, dV)
    a.eng.close()
    ne = p.ne
    score.check([O[ne], dS, dV], score.reference(p.rp_ne, p.ci, len(ne), K, Sn, Vn, Gn[ne], mode))
    empty_rows_ok(p, O, lse if mode == score.SOFTMAX else None)


@pytest.mark.parametrize("reduce", ["amax", "amin"])
@tiled_cases
def test_spmm_reduce(sx, N, name, reduce):
    """C and arg are bit-determined (ties included: the smaller entry wins), so the forward is compared exactly, empty rows (+0, -1) too"""
    p, rs = pat(name), rng("reduce", N, name, reduce)
    v, B, G = rand(rs, p.nnz), rand(rs, p.K, N), rand(rs, p.M, N)
    a = red.Abi(sx, p.rp, p.ci, v, p.M, p.K)
    wantC, wantA = red.ref_reduce(p.rp, p.ci, v, B, reduce)
    C, arg, _, _ = a.forward(reduce, B)
    fwd = a.eng.last_kernel()
    assert red.bits_equal(C, wantC) and np.array_equal(arg, wantA)
    assert np.all(C[p.empty].view(np.uint32) == 0) and np.all(arg[p.empty] == -1)
    dB, dv = a.backward(B, arg, G)
    names_ok(p, "spmm_reduce", fwd, a.eng.last_kernel())
    a.eng.close()
    wdB, wdv = red.ref_grads(p.ci, v, B, wantA, G, p.K)
    assert _close(dB, wdB), float(np.abs(dB - wdB).max())
    assert _close(dv, wdv), float(np.abs(dv - wdv).max())


@tiled_cases
def test_spmm_multi(sx, N, name):
    """all groups on: sum, sum of squares, max, min and both args"""
    p, rs = pat(name), rng("multi", N, name)
    v, B = rand(rs, p.nnz), rand(rs, p.K, N)
    G = {k: rand(rs, p.M, N) for k in multi.VALUES}
    a = multi.Abi(sx, p.rp, p.ci, v, p.M, p.K)
    got, _ = a.forward(B)
    fwd = a.eng.last_kernel()
    _, want = multi.reference(p.rp, p.ci, v, B)
    for k in ("max", "min"):
        assert multi.raw_equal(got[k], want[k]) and np.array_equal(got["arg" + k], want["arg" + k]), k
    assert multi.within_bound(got["sum"], want["sum"], want["abs"], p.lens, "sum")
    assert multi.within_bound(got["sumsq"], want["sumsq"], want["sumsq"], p.lens, "sumsq")
    for k in multi.VALUES:
        assert np.all(got[k][p.empty].view(np.uint32) == 0), k
    assert np.all(got["argmax"][p.empty] == -1) and np.all(got["argmin"][p.empty] == -1)
    args = {"max": got["argmax"], "min": got["argmin"]}
    w = multi.ref_backward(p.rp, p.ci, v, B, args, G, p.K)
    dB, dv = a.backward(B, args, G)
    names_ok(p, "spmm_multi", fwd, a.eng.last_kernel())
    a.eng.close()
    assert multi.grad_bound(dB, w["dB"], w["dB_abs"], w["dB_cnt"], "dB")
    assert multi.grad_bound(dv, w["dv"], w["dv_abs"], w["dv_cnt"], "dval")


@tiled_cases
def test_spmm_softagg(sx, N, name):
    p, rs = pat(name), rng("softagg", N, name)
    v, B, G, t = rand(rs, p.nnz), rand(rs, p.K, N), rand(rs, p.M, N), sagg.temps(N)
    a = sagg.SoftAbi(sx, p.rp, p.ci, v, p.M, p.K)
    C, lse, _, _ = a.fwd(B, t)
    fwd = a.eng.last_kernel()
    got = a.bwd(B, t, C, lse, G)
    names_ok(p, "spmm_softagg", fwd, a.eng.last_kernel())
    a.eng.close()
    wC, wL, wdB, wdv, wdt = sagg.reference(p.rp, p.ci, v, B, t, G, p.K)
    assert _close(C, wC), float(np.abs(C - wC).max())
    assert sagg.lse_close(lse, wL)
    for k, want in (("dB", wdB), ("dval", wdv), ("dt", wdt)):
        assert _close(got[k], want), (k, float(np.abs(got[k] - want).max()))
    empty_rows_ok(p, C, lse)


@pytest.mark.parametrize("op", ["mul", "add_relu"])
@tiled_cases
def test_spmm_edge(sx, N, name, op):
    """integer operands in [-4, 4]: every partial sum is an integer below 2^24, C, dB and dE equal the int64 computation"""
    p, rs = pat(name), rng("edge", N, name, op)
    B, E, G = sedge.ints(rs, p.K, N), sedge.ints(rs, p.nnz, N), sedge.ints(rs, p.M, N)
    a = sedge.Abi(sx, p.rp, p.ci, p.M, p.K)
    wC, wdB, wdE, _, _ = sedge.reference(op, p.rp, p.ci, B, E, G, p.K, dtype=np.int64)
    C, _ = a.forward(op, B, E)
    fwd = a.eng.last_kernel()
    dB, dE, _, _ = a.backward(op, B, E, G)
    names_ok(p, "spmm_edge", fwd, a.eng.last_kernel())
    a.eng.close()
    assert np.array_equal(C, wC.astype(np.float32))
    assert np.array_equal(dE, wdE.astype(np.float32)) and np.array_equal(dB, wdB.astype(np.float32))
    assert np.all(C[p.empty].view(np.uint32) == 0)


# --- 4. uniform scores, integer values: O = sum / n ----------------------------------------------------------------------------------------
def mean_is_exact(p, O, lse, values):
    """O (M, ..) against the int64 sum of the rows' integer `values` (nnz, ..) over n: within 4 * 2^-24 relative (one reciprocal or
    division and one multiply, about 1 ulp each in the hardware's fast forms), exactly 0 where the sum is 0; lse = log n"""
    rows = np.repeat(np.arange(p.M), p.lens)
    vals = np.asarray(values)
    assert np.all(vals == np.rint(vals)) and np.all(vals != 0) and np.abs(vals).max() * p.lens.max() < 2 ** 24
    sums = np.zeros((p.M,) + vals.shape[1:], np.int64)
    np.add.at(sums, rows, vals.astype(np.int64))
    n = p.lens.astype(np.float64).reshape((p.M,) + (1,) * (vals.ndim - 1))
    ne = p.ne
    want = sums[ne].astype(np.float64) / n[ne]
    got = O[ne].astype(np.float64)
    assert got.shape == want.shape
    err = np.abs(got - want)
    nz = want != 0
    print("max relative error / 2^-24:", float((err[nz] / np.abs(want[nz])).max() / 2.0 ** -24), "zero sums:", int(np.count_nonzero(~nz)))
    assert np.all(err <= 4 * 2.0 ** -24 * np.abs(want)), float((err[nz] / np.abs(want[nz])).max() / 2.0 ** -24)
    assert np.count_nonzero(~nz) == 0 or np.all(got[~nz] == 0)
    if lse is not None:
        logn = np.broadcast_to(np.log(n[ne]).reshape((len(ne),) + (1,) * (lse.ndim - 1)), lse[ne].shape)
        assert _close(lse[ne], logn), float(np.abs(lse[ne] - logn).max())
    empty_rows_ok(p, O, lse)


H4 = 3
sharp = lambda f: pytest.mark.parametrize("name", PATTERNS)(pytest.mark.parametrize("w", WIDTHS)(gpu(f)))   # noqa: E731


@sharp
def test_uniform_scores_fused_attention(sx, w, name):
    p, rs = pat(name), rng("u-attention", w, name)
    Qn, Kn, Vn = np.zeros((p.M, H4, w), np.float32), rand(rs, p.K, H4, w), int_values(rs, p.K, H4, w)
    a = att.Abi(sx, p.rp, p.ci, p.M, p.K, H4, w, w)
    O, lse = host(*a.forward(dev(Qn), dev(Kn), dev(Vn), None, SCALE))
    names_ok(p, "attention_fused", a.eng.last_kernel(), None)
    a.eng.close()
    mean_is_exact(p, O, lse, Vn[p.ci])


@sharp
def test_uniform_scores_attention_edge(sx, w, name):
    """the message is V[c] + Ev[e]: +-3, +-4 plus +-1, an integer of magnitude 2 .. 5"""
    p, rs = pat(name), rng("u-attention_edge", w, name)
    ops = dict(Q=np.zeros((p.M, H4, w), np.float32), K=rand(rs, p.K, H4, w), Ek=rand(rs, p.nnz, H4, w), b=None,
               V=(rs.randint(3, 5, (p.K, H4, w)) * rs.choice([-1, 1], (p.K, H4, w))).astype(np.float32),
               Ev=rs.choice([-1, 1], (p.nnz, H4, w)).astype(np.float32))
    a = aedge.Abi(sx, p.rp, p.ci, p.M, p.K, H4, w, w)
    got = a.run(ops, rand(rs, p.M, H4, w), SCALE)
    names_ok(p, "attention_edge_fused", a.fwd_kernel, None)
    a.eng.close()
    mean_is_exact(p, got["O"], got["lse"], ops["V"][p.ci] + ops["Ev"])


@sharp
def test_uniform_scores_gat(sx, w, name):
    p, rs = pat(name), rng("u-gat", w, name)
    adn, asn, Vn = np.zeros((p.M, H4), np.float32), np.zeros((p.K, H4), np.float32), int_values(rs, p.K, H4, w)
    a = gat.Abi(sx, p.rp, p.ci, p.M, p.K, H4, w)
    O, lse = host(*a.forward(dev(adn), dev(asn), dev(Vn), None, SLOPE))
    names_ok(p, "gat_fused", a.eng.last_kernel(), None)
    a.eng.close()
    mean_is_exact(p, O, lse, Vn[p.ci])


@sharp
def test_uniform_scores_gatv2(sx, w, name):
    """att = 0: every score is <0, leaky_relu(z)> = 0; the message is x_src"""
    p, rs = pat(name), rng("u-gatv2", w, name)
    xdn, xsn, attn = rand(rs, p.M, H4, w), int_values(rs, p.K, H4, w), np.zeros((H4, w), np.float32)
    a = gatv2.Abi(sx, p.rp, p.ci, p.M, p.K, H4, w)
    O, lse = host(*a.forward(dev(xdn), dev(xsn), dev(attn), None, SLOPE))
    names_ok(p, "gatv2_fused", a.eng.last_kernel(), None)
    a.eng.close()
    mean_is_exact(p, O, lse, xsn[p.ci])


@sharp
def test_uniform_scores_score_attention(sx, w, name):
    p, rs = pat(name), rng("u-score", w, name)
    Sn, Vn = np.zeros((p.nnz, H4), np.float32), int_values(rs, p.K, H4, w)
    a = score.Abi(sx, p.rp, p.ci, p.M, p.K, H4, w)
    O, lse = host(*a.forward(score.SOFTMAX, dev(Sn), dev(Vn)))
    names_ok(p, "score_softmax_fused", a.eng.last_kernel(), None)
    a.eng.close()
    mean_is_exact(p, O, lse, Vn[p.ci])


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("N", TILED)
@gpu
def test_uniform_scores_softagg(sx, N, name):
    """t = 0 and val = +-1: the messages are +-B[c], their weights 1 / n"""
    p, rs = pat(name), rng("u-softagg", N, name)
    v, B = rs.choice([-1, 1], p.nnz).astype(np.float32), int_values(rs, p.K, N)
    a = sagg.SoftAbi(sx, p.rp, p.ci, v, p.M, p.K)
    C, lse, _, _ = a.fwd(B, np.zeros(N, np.float32))
    names_ok(p, "spmm_softagg", a.eng.last_kernel(), None)
    a.eng.close()
    mean_is_exact(p, C, lse, v[:, None] * B[p.ci])


# --- 5. the dropout variants ---------------------------------------------------------------------------------------------------------------
DROP_P, DROP_SEED = 0.5, 20240


def dropout_operands(fam, rs, p, H, w):
    """the three operands of drp.Abi / drp.reference, LeakyReLU's kink avoided by the grid"""
    if fam == "attention":
        return [rand(rs, p.M, H, w), rand(rs, p.K, H, w), rand(rs, p.K, H, w)]
    if fam == "gat":
        ops = list(gat_scores(rs, p.M, p.K, H)) + [rand(rs, p.K, H, w)]
        gat.assert_off_the_kink(p.rp, p.ci, ops[0], ops[1])
        return ops
    ops = [grid(rs, p.M, H, w, False), grid(rs, p.K, H, w, True), rand(rs, H, w)]
    gatv2.assert_off_the_kink(p.rp, p.ci, ops[0], ops[1])
    return ops


def device_mult(p, H, prob, seed):
    """(nnz, H) multipliers of torch_op.dropout_mask on the pattern"""
    from sextans_amd import torch_op
    torch_op.clear_cache()
    mult = torch_op.dropout_mask(make_A(p.rp, p.ci, np.ones(p.nnz, np.float32), p.M, p.K), H, prob, seed).cpu().numpy()
    torch_op.clear_cache()
    assert mult.shape == (p.nnz, H) and 0.3 < np.mean(mult == 0) < 0.7
    return mult


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("w", [8, 128])
@pytest.mark.parametrize("fam", drp.FAMILIES)
@gpu
def test_dropout(sx, fam, w, name):
    p, rs = pat(name), rng("dropout", fam, w, name)
    H = 3
    ops, Gn = dropout_operands(fam, rs, p, H, w), rand(rs, p.M, H, w)
    mult = device_mult(p, H, DROP_P, DROP_SEED)
    a = drp.Abi(sx, fam, p.rp, p.ci, p.M, p.K, H, w)
    got = a.everything([dev(x) for x in ops], None, sx.api.Dropout(DROP_P, DROP_SEED), dev(Gn))
    names_ok(p, drp.ENTRY[fam].replace("_attention", "") + "_fused", a.fwd_kernel, a.bwd_kernel, dropout=True)
    a.eng.close()
    drp.compare(fam, got, drp.reference(fam, p.rp, p.ci, p.M, p.K, ops, Gn, None, mult), p.rp, False)


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("fam", drp.FAMILIES)
@gpu
def test_dropout_zero_is_the_plain_call(sx, fam, name):
    """p = 0 with a Dropout struct: the plain kernels, the plain bits (width 128)"""
    p, rs = pat(name), rng("dropout0", fam, name)
    H, w = 3, 128
    ops, G = [dev(x) for x in dropout_operands(fam, rs, p, H, w)], dev(rand(rs, p.M, H, w))
    a = drp.Abi(sx, fam, p.rp, p.ci, p.M, p.K, H, w)
    plain = a.everything(ops, None, None, G, plain=True)
    names_ok(p, drp.ENTRY[fam].replace("_attention", "") + "_fused", a.fwd_kernel, a.bwd_kernel)
    zero = a.everything(ops, None, sx.api.Dropout(0.0, DROP_SEED), G)
    names_ok(p, drp.ENTRY[fam].replace("_attention", "") + "_fused", a.fwd_kernel, a.bwd_kernel)
    a.eng.close()
    assert len(plain) == len(zero) and all(same(x, y) for x, y in zip(plain, zero))


def score_run(p, Sn, Vn, Gn, **kw):
    """score.run through torch_op -> (O, dS, dV), the names of the forward's and the backward's kernel"""
    import torch
    from sextans_amd import torch_op
    torch_op.clear_cache()
    v = np.ones(p.nnz, np.float32)
    got = score.run(p.rp, p.ci, v, p.M, p.K, Sn, Vn, Gn, score.SOFTMAX, **kw)
    bwd = list(torch_op._cache.values())[-1].eng.last_kernel()
    with torch.no_grad():
        torch_op.score_attention(make_A(p.rp, p.ci, v, p.M, p.K), dev(Sn), dev(Vn), **kw)
    fwd = list(torch_op._cache.values())[-1].eng.last_kernel()
    torch_op.clear_cache()
    return got, fwd, bwd


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("w", [8, 128])
@gpu
def test_dropout_score_attention(sx, w, name):
    p, rs = pat(name), rng("dropout-score", w, name)
    H = 3
    Sn, Vn, Gn = score.scores(rs, p.nnz, H, score.SOFTMAX), rand(rs, p.K, H, w), rand(rs, p.M, H, w)
    mult = device_mult(p, H, DROP_P, DROP_SEED)
    got, fwd, bwd = score_run(p, Sn, Vn, Gn, dropout=DROP_P, seed=DROP_SEED)
    names_ok(p, "score_softmax_fused", fwd, bwd, dropout=True)
    ne = p.ne
    score.check([got[0][ne], got[1], got[2]], score.reference(p.rp_ne, p.ci, len(ne), p.K, Sn, Vn, Gn[ne], score.SOFTMAX, mult))
    empty_rows_ok(p, got[0])


@pytest.mark.parametrize("name", PATTERNS)
@gpu
def test_dropout_zero_is_the_plain_call_score_attention(sx, name):
    p, rs = pat(name), rng("dropout0-score", name)
    H, w = 3, 128
    Sn, Vn, Gn = score.scores(rs, p.nnz, H, score.SOFTMAX), rand(rs, p.K, H, w), rand(rs, p.M, H, w)
    plain, fwd, bwd = score_run(p, Sn, Vn, Gn)
    names_ok(p, "score_softmax_fused", fwd, bwd)
    zero, fwd, bwd = score_run(p, Sn, Vn, Gn, dropout=0.0, seed=DROP_SEED)
    names_ok(p, "score_softmax_fused", fwd, bwd)
    assert all(same(x, y) for x, y in zip(plain, zero))
