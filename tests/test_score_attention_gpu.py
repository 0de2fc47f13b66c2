"""score_attention and the C ABI under it (sextans_score_attention_device, sextans_score_attention_backward_device): attention from
caller-supplied (nnz, H) scores -- softmax per row and head, or the raw weights -- in one kernel pass per direction, against the float64
dense masked computation per head (O, dS, dV) with the tolerance every fused attention here is held to
(test_torch_autograd_gpu._close, rtol 2e-4); row lengths around every lane-group size and beyond the long-row threshold; the bits of the
GAT kernels when fed GAT's scores; empty rows, unused columns, -inf masks, skipped passes and strided S on the C ABI; the two modes
against each other and against spmm; dropout and a captured training step."""
import numpy as np
import pytest

from test_fused_attention_gpu import edge_pattern, rand, same
from test_gat_attention_gpu import Abi as GatAbi
from test_gat_attention_gpu import assert_off_the_kink
from test_torch_attention_gpu import make_A, pattern
from test_torch_autograd_gpu import _close

pytestmark = pytest.mark.gpu

LR = 0.05
INVALID = 9
SOFTMAX, WEIGHT = 1, 2
NORMALIZE = {SOFTMAX: "softmax", WEIGHT: "none"}


def reference(rp, ci, M, K, Sn, Vn, Gn, mode, mult=None):
    """float64 dense masked computation head by head: O (M, H, dv), dS (nnz, H), dV (K, H, dv).  mult: (nnz, H) dropout multipliers on
    the normalised coefficients"""
    import torch
    H = Vn.shape[1]
    rows = torch.from_numpy(np.repeat(np.arange(M), np.diff(rp))).cuda()
    cols = torch.from_numpy(ci.astype(np.int64)).cuda()
    mask = torch.full((M, K), float("-inf"), dtype=torch.float64, device="cuda")
    mask[rows, cols] = 0.0
    out = {k: [] for k in ("O", "dS", "dV")}
    for h in range(H):
        s, V = (torch.from_numpy(np.ascontiguousarray(t[:, h])).cuda().double().requires_grad_() for t in (Sn, Vn))
        D = torch.zeros((M, K), dtype=torch.float64, device="cuda").index_put((rows, cols), s)
        if mode == SOFTMAX:
            D = torch.softmax(D + mask, dim=1)
            if mult is not None:
                D = D * torch.zeros((M, K), dtype=torch.float64, device="cuda").index_put((rows, cols), torch.from_numpy(mult[:, h]).cuda().double())
        O = D @ V
        O.backward(torch.from_numpy(np.ascontiguousarray(Gn[:, h])).cuda().double())
        out["O"].append(O.detach().cpu().numpy()); out["dS"].append(s.grad.cpu().numpy()); out["dV"].append(V.grad.cpu().numpy())
    return {k: np.stack(x, axis=1) for k, x in out.items()}


def run(rp, ci, v, M, K, Sn, Vn, Gn, mode, squeeze=False, **kw):
    """-> (O, dS, dV) as numpy, heads on axis 1; squeeze: hand H = 1 operands over as (nnz,) and (rows, dv)"""
    import torch
    from sextans_amd import torch_op
    A = make_A(rp, ci, v, M, K)
    S, V = (torch.from_numpy(t[:, 0] if squeeze else t).cuda().requires_grad_() for t in (Sn, Vn))
    out = torch_op.score_attention(A, S, V, normalize=NORMALIZE[mode], **kw)
    assert out.dim() == V.dim()
    out.backward(torch.from_numpy(Gn[:, 0] if squeeze else Gn).cuda())
    assert S.grad.shape == S.shape and V.grad.shape == V.shape and S.grad.dtype == S.dtype
    res = [t.detach().cpu().numpy() for t in (out, S.grad, V.grad)]
    return [t[:, None] for t in res] if squeeze else res


def check(got, want):
    for g, k in zip(got, ("O", "dS", "dV")):
        assert g.shape == want[k].shape, k
        assert np.all(np.isfinite(g)), k
        print(k, "max |got - want|", float(np.abs(g - want[k]).max()), "max |want|", float(np.abs(want[k]).max()))
        assert _close(g, want[k]), (k, float(np.abs(g - want[k]).max()))


def scores(rs, nnz, H, mode):
    """WEIGHT: uniform(-1, 1) weights; SOFTMAX: scores a few units apart, so that the coefficients of a row differ by orders of magnitude"""
    return rand(rs, nnz, H) if mode == WEIGHT else (3.0 * rand(rs, nnz, H)).astype(np.float32)


@pytest.mark.parametrize("mode", [SOFTMAX, WEIGHT])
@pytest.mark.parametrize("H, dv", [(1, 16), (3, 24), (2, 40), (2, 64), (1, 128), (2, 8)])
def test_against_dense_float64(sx, H, dv, mode):
    from sextans_amd import torch_op
    M, K = 300, 260
    rs, rp, ci, v = pattern(31 + dv, M, K, 9)
    assert np.all(np.diff(rp) > 0)
    Sn, Vn, Gn = scores(rs, len(ci), H, mode), rand(rs, K, H, dv), rand(rs, M, H, dv)
    torch_op.clear_cache()
    got = run(rp, ci, v, M, K, Sn, Vn, Gn, mode, squeeze=(H == 1 and dv == 16))
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0, info
    check(got, reference(rp, ci, M, K, Sn, Vn, Gn, mode))
    torch_op.clear_cache()


@pytest.mark.parametrize("mode", [SOFTMAX, WEIGHT])
def test_row_length_edges_and_long_rows(sx, mode):
    import torch
    from sextans_amd import torch_op
    rs = np.random.RandomState(8)
    rp, ci, v, M, K = edge_pattern(rs)
    assert M < 3000 and np.count_nonzero(ci == 0) > 2048 and np.diff(rp).max() == 2500
    H, dv = 2, 16
    Sn, Vn, Gn = scores(rs, len(ci), H, mode), rand(rs, K, H, dv), rand(rs, M, H, dv)
    name = "score_softmax_fused" if mode == SOFTMAX else "score_weight_fused"
    torch_op.clear_cache()
    got = run(rp, ci, v, M, K, Sn, Vn, Gn, mode)
    eng = next(iter(torch_op._cache.values())).eng
    assert eng.last_kernel() == name + "_backward+long_rows"
    check(got, reference(rp, ci, M, K, Sn, Vn, Gn, mode))
    ones = np.flatnonzero(np.diff(rp) == 1)
    assert len(ones) == 2101
    if mode == SOFTMAX:   # a row of one entry: p = 1, O is V's row, <G, V> - delta cancels exactly
        assert same(got[0][ones], Vn[ci[rp[ones]]])
        assert np.all(got[1][rp[ones]] == 0)
    else:                 # the float32 product of the weight and V's row
        assert same(got[0][ones], Sn[rp[ones]][:, :, None] * Vn[ci[rp[ones]]])
    # the forward alone names its own kernel
    A = make_A(rp, ci, v, M, K)
    torch_op.score_attention(A, *(torch.from_numpy(t).cuda() for t in (Sn, Vn)), normalize=NORMALIZE[mode])
    assert list(torch_op._cache.values())[-1].eng.last_kernel() == name + "+long_rows"   # (A's new index tensors: a new entry)
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

    def forward(self, mode, S, V, drop=None, lds=None):
        t, H, dv = self.t, self.H, self.dv
        O = t.full((self.M, H, dv), 7.0, device="cuda"); lse = t.full((self.M, H), 7.0, device="cuda")
        self.eng.score_attention_device(mode, H, dv, S.data_ptr(), lds or H, V.data_ptr(), H * dv, O.data_ptr(), H * dv, lse.data_ptr(), drop,
                                        t.cuda.current_stream().cuda_stream)
        return O, lse

    def backward(self, mode, S, V, O, lse, G, drop=None, lds=None, want_dS=True, want_dV=True, dS=None, ldds=None):
        t, H, dv = self.t, self.H, self.dv
        if dS is None and want_dS:
            dS = t.full((max(self.nnz, 1), H), 7.0, device="cuda")
        dV = t.full((self.K, H, dv), 7.0, device="cuda") if want_dV else None
        self.eng.score_attention_backward_device(mode, H, dv, S.data_ptr(), lds or H, V.data_ptr(), H * dv, O.data_ptr(), H * dv, lse.data_ptr(),
                                                 G.data_ptr(), H * dv, dS.data_ptr() if want_dS else None, ldds or H,
                                                 dV.data_ptr() if want_dV else None, H * dv, drop, t.cuda.current_stream().cuda_stream)
        return (dS[:self.nnz] if want_dS else None), dV


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_the_bits_of_the_gat_kernels_on_gat_scores(sx, p):
    """S[e, h] = leaky_relu(a_dst[r, h] + a_src[c, h]) made in float32 as the GAT kernels make it: from s onward the two families do the
    same arithmetic in the same order, so O, lse and dV agree bit for bit; dS summed over a row, times the activation's slope per
    entry, is GAT's d a_dst up to rounding."""
    import torch
    rs = np.random.RandomState(8)
    rp, ci, _, M, K = edge_pattern(rs)
    H, dv, slope = 2, 16, 0.2
    adn, asn, Vn, Gn = rand(rs, M, H), rand(rs, K, H), rand(rs, K, H, dv), rand(rs, M, H, dv)
    assert_off_the_kink(rp, ci, adn, asn)
    rows = np.repeat(np.arange(M), np.diff(rp))
    z = adn[rows] + asn[ci]
    assert z.dtype == np.float32
    Sn = np.where(z > 0, z, np.float32(slope) * z).astype(np.float32)
    ad, as_, V, G, S = (torch.from_numpy(t).cuda() for t in (adn, asn, Vn, Gn, Sn))
    step = torch.tensor([3], dtype=torch.int64, device="cuda")
    drop = sx.api.Dropout(p, 77, step.data_ptr()) if p else None
    stream = torch.cuda.current_stream().cuda_stream
    g, a = GatAbi(sx, rp, ci, M, K, H, dv), Abi(sx, rp, ci, M, K, H, dv)
    # GAT through its own entry points (the dropout entries with a Dropout)
    gO, glse = torch.full((M, H, dv), 7.0, device="cuda"), torch.full((M, H), 7.0, device="cuda")
    fwd = (H, dv, slope, ad.data_ptr(), H, as_.data_ptr(), H, V.data_ptr(), H * dv, None, gO.data_ptr(), H * dv, glse.data_ptr())
    delta, dad, das = (torch.full((n, H), 7.0, device="cuda") for n in (M, M, K))
    gdV = torch.full((K, H, dv), 7.0, device="cuda")
    bwd = fwd[:10] + (gO.data_ptr(), H * dv, glse.data_ptr(), G.data_ptr(), H * dv, delta.data_ptr(), dad.data_ptr(), H, das.data_ptr(), H,
                      gdV.data_ptr(), H * dv, None)
    if drop is None:
        g.eng.gat_attention_device(*fwd, stream)
        g.eng.gat_attention_backward_device(*bwd, stream)
    else:
        g.eng.gat_attention_dropout_device(*fwd, drop, stream)
        g.eng.gat_attention_dropout_backward_device(*bwd, drop, stream)
    O, lse = a.forward(SOFTMAX, S, V, drop)
    dS, dV = a.backward(SOFTMAX, S, V, O, lse, G, drop)
    assert a.eng.last_kernel() == "score_softmax_fused_backward" + ("+dropout" if p else "") + "+long_rows"
    n = lambda x: x.cpu().numpy()   # noqa: E731
    assert same(n(O), n(gO)) and same(n(lse), n(glse)) and same(n(dV), n(gdV))
    dz = n(dS).astype(np.float64) * np.where(z > 0, 1.0, slope)
    mine = np.stack([np.bincount(rows, dz[:, h], minlength=M) for h in range(H)], axis=1)
    assert _close(mine, n(dad)), float(np.abs(mine - n(dad)).max())
    g.eng.close(); a.eng.close()


@pytest.mark.parametrize("mode", [SOFTMAX, WEIGHT])
def test_empty_rows_masks_skipped_passes_and_strides_on_the_c_abi(sx, mode):
    import torch
    from util import random_csr
    rs = np.random.RandomState(17)
    M, K, H, dv = 400, 400, 2, 24
    rp, ci, _ = random_csr(rs, M, K - 20, 6, empty_frac=0.2)   # the last 20 columns have no entry
    lens = np.diff(rp)
    empty = np.flatnonzero(lens == 0)
    assert len(empty) > 20
    nnz = len(ci)
    Sn, Vn, Gn = scores(rs, nnz, H, mode), rand(rs, K, H, dv), rand(rs, M, H, dv)
    multi = np.flatnonzero(lens >= 2)
    dead = int(np.flatnonzero(lens == 3)[0])
    masked = rp[multi[multi != dead]]
    if mode == SOFTMAX:
        # rows of two or more entries: their first entry is masked out (-inf) in both heads; one row of three is masked out completely
        # in head 0 alone
        Sn[masked] = -np.inf
        Sn[rp[dead]:rp[dead + 1], 0] = -np.inf
    S, V, G = (torch.from_numpy(t).cuda() for t in (Sn, Vn, Gn))
    a = Abi(sx, rp, ci, M, K, H, dv)
    O, lse = a.forward(mode, S, V)
    dS, dV = a.backward(mode, S, V, O, lse, G)
    assert a.eng.last_kernel() == ("score_softmax_fused_backward" if mode == SOFTMAX else "score_weight_fused_backward")
    On, lsen, dSn, dVn = (x.cpu().numpy() for x in (O, lse, dS, dV))
    # everything is written (the buffers held 7.0); empty rows: O = +0 (the bits), lse = -inf; columns without entries: dV = 0
    assert not np.any(On == 7.0) and not np.any(dSn == 7.0) and not np.any(dVn == 7.0)
    assert np.all(On[empty].view(np.uint32) == 0) and np.all(dVn[K - 20:] == 0)
    if mode == SOFTMAX:
        assert not np.any(lsen == 7.0) and np.all(lsen[empty] == -np.inf)
        # the (row, head) whose scores are all -inf is NaN, and nothing else is
        fin = np.ones((M, H), bool); fin[dead, 0] = False
        assert np.all(np.isnan(On[dead, 0])) and np.all(np.isfinite(On[fin]))
        efin = np.ones((nnz, H), bool); efin[rp[dead]:rp[dead + 1], 0] = False
        assert np.all(np.isnan(dSn[~efin])) and np.all(np.isfinite(dSn[efin]))
        assert np.all(np.isfinite(lsen[fin & (lens > 0)[:, None]]))
        # (the dead row's NaN reaches dV in head 0 of its columns: the others -- they are most -- are finite)
        clean = np.ones((K, H), bool); clean[ci[rp[dead]:rp[dead + 1]], 0] = False
        assert np.all(np.isfinite(dVn[clean]))
        # a -inf entry beside finite ones contributes exactly 0: dS is 0 there; a row of [-inf, s] gives the bits of V's row of its second
        # entry; and the results are those of the pattern without the masked entries
        assert np.all(dSn[masked] == 0)
        two = np.flatnonzero(lens == 2)
        assert len(two) > 3 and same(On[two], Vn[ci[rp[two] + 1]])
        keep = np.ones(nnz, bool); keep[masked] = False
        rows = np.repeat(np.arange(M), lens)
        rp2 = np.zeros(M + 1, np.int32); rp2[1:] = np.cumsum(np.bincount(rows[keep], minlength=M))
        b = Abi(sx, rp2, ci[keep], M, K, H, dv)
        S2 = torch.from_numpy(Sn[keep]).cuda()
        O2, lse2 = b.forward(mode, S2, V)
        dS2, dV2 = b.backward(mode, S2, V, O2, lse2, G)
        O2n, lse2n, dS2n, dV2n = (x.cpu().numpy() for x in (O2, lse2, dS2, dV2))
        have = fin & (lens > 0)[:, None]
        assert _close(On[fin], O2n[fin]) and _close(lsen[have], lse2n[have])
        assert _close(dSn[keep][efin[keep]], dS2n[efin[keep]]) and _close(dVn[clean], dV2n[clean])
        b.eng.close()
    # d_dS = NULL / d_dV = NULL: that pass is skipped, the other's bits are the same
    _, dV_only = a.backward(mode, S, V, O, lse, G, want_dS=False)
    dS_only, _ = a.backward(mode, S, V, O, lse, G, want_dV=False)
    assert same(dV_only.cpu().numpy(), dVn) and same(dS_only.cpu().numpy(), dSn)
    with pytest.raises(sx.api.SextansError) as err:
        a.backward(mode, S, V, O, lse, G, want_dS=False, want_dV=False)
    assert err.value.code == INVALID
    # S and dS as columns [4, 4 + H) of wider buffers: the same bits, and nothing beside dS's columns is written
    pad = H + 6
    Sw = torch.full((nnz, pad), 9.0, device="cuda"); Sw[:, 4:4 + H] = S
    dSw = torch.full((nnz, pad), 7.0, device="cuda")
    Sv, dSv = Sw[:, 4:], dSw[:, 4:]
    assert Sv.data_ptr() % 16 == 0 and dSv.data_ptr() % 16 == 0
    O3, lse3 = a.forward(mode, Sv, V, lds=pad)
    dS3, dV3 = a.backward(mode, Sv, V, O3, lse3, G, lds=pad, dS=dSv, ldds=pad)
    assert same(O3.cpu().numpy(), On) and same(dV3.cpu().numpy(), dVn) and same(dSw[:, 4:4 + H].cpu().numpy(), dSn)
    if mode == SOFTMAX:
        assert same(lse3.cpu().numpy(), lsen)
    rest = dSw.cpu().numpy().copy(); rest[:, 4:4 + H] = 7.0
    assert np.all(rest == 7.0)
    # a NULL operand with nnz > 0 is refused
    with pytest.raises(sx.api.SextansError) as err:
        a.eng.score_attention_device(mode, H, dv, S.data_ptr(), H, None, H * dv, O.data_ptr(), H * dv, lse.data_ptr(), None, None)
    assert err.value.code == INVALID
    # no entries at all: everything is written, nothing is launched on the pattern
    c = Abi(sx, np.zeros(M + 1, np.int32), np.zeros(0, np.int32), M, K, H, dv)
    O4, lse4 = c.forward(mode, S, V)
    _, dV4 = c.backward(mode, S, V, O4, lse4, G)
    assert np.all(O4.cpu().numpy().view(np.uint32) == 0) and np.all(dV4.cpu().numpy() == 0)
    if mode == SOFTMAX:
        assert np.all(lse4.cpu().numpy() == -np.inf)
    for e in (a, c):
        e.eng.close()


def test_the_two_modes_agree_and_weight_mode_is_spmm(sx):
    import torch
    from sextans_amd import torch_op
    M, K, H, dv = 300, 260, 3, 24
    rs, rp, ci, v = pattern(61, M, K, 9)
    Sn, Vn = scores(rs, len(ci), H, SOFTMAX), rand(rs, K, H, dv)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    S, V = torch.from_numpy(Sn).cuda(), torch.from_numpy(Vn).cuda()
    rows = torch_op.entry_rows(A)
    assert rows.dtype == torch.int64 and np.array_equal(rows.cpu().numpy(), np.repeat(np.arange(M), np.diff(rp)))
    out, w = torch_op.score_attention(A, S, V, return_weights=True)
    assert w.shape == S.shape and not w.requires_grad
    sums = torch.zeros((M, H), device="cuda").index_add_(0, rows, w).cpu().numpy()
    assert np.all(np.abs(sums - 1.0) < 1e-5)
    again = torch_op.score_attention(A, w, V, normalize="none")
    assert _close(again.cpu().numpy(), out.cpu().numpy())
    # 1-D operands; H = 1 with A's own values as the weights is spmm
    V1 = V[:, 0].contiguous()
    o1, w1 = torch_op.score_attention(A, S[:, 0].contiguous(), V1, return_weights=True)
    assert w1.shape == (len(ci),) and o1.shape == (M, dv)
    assert _close(o1.cpu().numpy(), out[:, 0].cpu().numpy())   # (one head alone is dealt to other lane groups: not the same bits)
    got = torch_op.score_attention(A, A.values(), V1, normalize="none")
    assert _close(got.cpu().numpy(), torch_op.spmm(A, V1).cpu().numpy())
    with pytest.raises(ValueError):
        torch_op.score_attention(A, S, V, normalize="none", dropout=0.5)
    with pytest.raises(ValueError):
        torch_op.score_attention(A, S, V, normalize="none", return_weights=True)
    with pytest.raises(ValueError):
        torch_op.score_attention(A, S, V, normalize="l1")
    with pytest.raises(ValueError):
        torch_op.score_attention(A, S[:, :2], V)
    with pytest.raises(ValueError):
        torch_op.score_attention(A, S[:-1], V)
    torch_op.clear_cache()


def test_dropout(sx):
    import torch
    from sextans_amd import torch_op
    M, K, H, dv, p, seed = 300, 260, 2, 24, 0.5, 4321
    rs, rp, ci, v = pattern(71, M, K, 9)
    Sn, Vn, Gn = scores(rs, len(ci), H, SOFTMAX), rand(rs, K, H, dv), rand(rs, M, H, dv)
    torch_op.clear_cache()
    plain = run(rp, ci, v, M, K, Sn, Vn, Gn, SOFTMAX)
    zero = run(rp, ci, v, M, K, Sn, Vn, Gn, SOFTMAX, dropout=0.0, seed=seed)
    assert all(same(x, y) for x, y in zip(plain, zero))
    assert list(torch_op._cache.values())[-1].eng.last_kernel() == "score_softmax_fused_backward"
    step = torch.tensor([2], dtype=torch.int64, device="cuda")
    one = run(rp, ci, v, M, K, Sn, Vn, Gn, SOFTMAX, dropout=p, seed=seed, step=step)
    assert list(torch_op._cache.values())[-1].eng.last_kernel() == "score_softmax_fused_backward+dropout"
    two = run(rp, ci, v, M, K, Sn, Vn, Gn, SOFTMAX, dropout=p, seed=seed, step=step)
    assert all(same(x, y) for x, y in zip(one, two))
    assert not same(one[0], plain[0])
    mult = torch_op.dropout_mask(make_A(rp, ci, v, M, K), H, p, seed, step).cpu().numpy()
    assert 0.3 < np.mean(mult == 0) < 0.7
    check(one, reference(rp, ci, M, K, Sn, Vn, Gn, SOFTMAX, mult))
    torch_op.clear_cache()


def test_captured_training_step_with_a_new_mask_per_replay(sx):
    """forward, backward and an SGD update of S and V in place, with dropout whose step counter moves inside the step; captured once and
    replayed three times: bit for bit three eager steps, on one engine."""
    import torch
    from sextans_amd import torch_op
    M, K, H, dv, p, seed = 900, 900, 2, 16, 0.5, 99
    rs, rp, ci, v = pattern(21, M, K, 10)
    Sn, Vn, Gn = scores(rs, len(ci), H, SOFTMAX), rand(rs, K, H, dv), rand(rs, M, H, dv)
    G = torch.from_numpy(Gn).cuda()

    def start():
        return make_A(rp, ci, v, M, K), [torch.from_numpy(t).cuda().requires_grad_() for t in (Sn, Vn)], torch.zeros(1, dtype=torch.int64, device="cuda")

    def step(A, params, counter):
        for t in params:
            t.grad = None
        out = torch_op.score_attention(A, *params, dropout=p, seed=seed, step=counter)
        out.backward(G)
        with torch.no_grad():
            for t in params:
                t.sub_(LR * t.grad)
            counter.add_(1)
        return out

    def state(out, params):
        return [out.detach().cpu().numpy().copy()] + [t.detach().cpu().numpy().copy() for t in params]

    torch_op.clear_cache()
    A, params, counter = start()
    eager = [state(step(A, params, counter), params) for _ in range(4)]
    assert not np.array_equal(eager[3][1], eager[0][1])
    torch_op.clear_cache()
    A, params, counter = start()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(A, params, counter)          # warm-up: engine, softmax tables, A^T and its tables
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step(A, params, counter)
    assert torch_op.cache_info()["engines_built"] == 1 and torch_op.cache_info()["value_refreshes"] == 0
    for k in range(1, 4):
        g.replay()
        torch.cuda.synchronize()
        got = state(out, params)
        for i in range(3):
            assert same(got[i], eager[k][i]), (k, i)
    assert int(counter.item()) == 4
    torch_op.clear_cache()
