"""Attention dropout inside the fused attention, GAT and GATv2 kernels (sextans_*_dropout_device, torch_op.*_dropout): every test runs
for the three families.  The mask of the float64 reference comes from the host (sextans_dropout_keep_host), never from the device.
  The reference is the float64 computation on the edge list with torch autograd (what test_gatv2_attention_gpu.reference does; a dense
masked softmax has no answer for the empty rows these patterns hold on purpose): scores, softmax over every row's entries, the
probabilities multiplied by the mask, the messages summed.  Tolerance: test_torch_autograd_gpu._close, the one the fused kernels are held
to without dropout.  LeakyReLU's kink is avoided as in the GAT and GATv2 tests (asserted on the CPU)."""
import numpy as np
import pytest

from test_fused_attention_gpu import rand, same
from test_gat_attention_gpu import assert_off_the_kink as gat_off_the_kink
from test_gatv2_attention_gpu import assert_off_the_kink as gatv2_off_the_kink
from test_gatv2_attention_gpu import grid
from test_torch_attention_gpu import make_A, pattern
from test_torch_autograd_gpu import _close
from util import random_csr

pytestmark = pytest.mark.gpu

FAMILIES = ("attention", "gat", "gatv2")
ENTRY = {"attention": "attention", "gat": "gat_attention", "gatv2": "gatv2_attention"}
GRADS = {"attention": ("dQ", "dK", "dV"), "gat": ("dadst", "dasrc", "dV"), "gatv2": ("dx_dst", "dx_src", "datt")}
SCALE, SLOPE = 0.37, 0.2
M64 = (1 << 64) - 1


def operands(fam, rs, M, K, H, d, rp, ci, bias):
    """the three operands of a family as numpy, LeakyReLU's kink avoided"""
    if fam == "attention":
        return [rand(rs, M, H, d), rand(rs, K, H, d), rand(rs, K, H, d)]
    if fam == "gat":
        ops = [rand(rs, M, H), rand(rs, K, H), rand(rs, K, H, d)]
        gat_off_the_kink(rp, ci, ops[0], ops[1], bias)
        return ops
    ops = [grid(rs, M, H, d, False), grid(rs, K, H, d, True), rand(rs, H, d)]
    gatv2_off_the_kink(rp, ci, ops[0], ops[1])
    return ops


def host_mult(nnz, H, p, seed, step=0):
    """(nnz, H) float32 multipliers from the host mask: 1.0f / (1.0f - p) in two rounded fp32 operations, or 0"""
    from sextans_amd import api
    keep = api.dropout_keep_host(0, nnz, H, p, seed, step)
    inv = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return keep.astype(np.float32) * inv


def reference(fam, rp, ci, M, K, ops, Gn, bias, mult):
    """float64 on the edge list -> {"O", "lse", "delta", "grads": [3], "dbias"}; mult: (nnz, H) multipliers or None"""
    import torch
    F = torch.nn.functional
    rows = torch.from_numpy(np.repeat(np.arange(M), np.diff(rp)).astype(np.int64))
    cols = torch.from_numpy(ci.astype(np.int64))
    t = [torch.from_numpy(x).double().requires_grad_() for x in ops]
    b = torch.from_numpy(bias).double().requires_grad_() if bias is not None else None
    H = Gn.shape[1]
    badd = b[:, None] if b is not None else 0.0
    if fam == "attention":
        s = SCALE * ((t[0][rows] * t[1][cols]).sum(-1) + badd)
        msg = t[2]
    elif fam == "gat":
        s = F.leaky_relu(t[0][rows] + t[1][cols] + badd, SLOPE)
        msg = t[2]
    else:
        s = (F.leaky_relu(t[0][rows] + t[1][cols], SLOPE) * t[2][None]).sum(-1) + badd
        msg = t[1]
    idx = rows[:, None].expand(-1, H)
    m = torch.full((M, H), float("-inf"), dtype=torch.float64).scatter_reduce(0, idx, s.detach(), "amax", include_self=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.exp(s - m[rows])
    Z = torch.zeros((M, H), dtype=torch.float64).index_add(0, rows, e)
    pr = e / Z[rows]
    if mult is not None:
        pr = pr * torch.from_numpy(mult).double()
    O = torch.zeros((M, H, msg.shape[-1]), dtype=torch.float64).index_add(0, rows, pr[:, :, None] * msg[cols])
    G = torch.from_numpy(Gn).double()
    O.backward(G)
    n = lambda x: x.detach().numpy()   # noqa: E731
    return {"O": n(O), "lse": n(m + torch.log(Z)), "delta": n((O * G).sum(-1)), "grads": [n(x.grad) for x in t],
            "dbias": n(b.grad) if b is not None else None}


class Abi:
    """one engine on a pattern; the entry points of a family called through api.Engine, with a Dropout, with None, or (plain) the entry
    without dropout"""

    def __init__(self, sx, fam, rp, ci, M, K, H, d):
        import torch
        self.t, self.sx, self.fam = torch, sx, fam
        self.M, self.K, self.H, self.d, self.nnz = M, K, H, d, len(ci)
        self.rp, self.ci = torch.from_numpy(rp.astype(np.int32)).cuda(), torch.from_numpy(ci.astype(np.int32)).cuda()
        self.val = torch.full((max(len(ci), 1),), float("nan"), device="cuda")   # A's own values are not read
        self.eng = sx.Engine(0)
        self.eng.set_matrix_csr_device(M, K, len(ci), self.rp.data_ptr(), self.ci.data_ptr(), self.val.data_ptr())

    def _lead(self, ops, bias):
        H, d = self.H, self.d
        a, b, c = (x.data_ptr() for x in ops)
        bp = bias.data_ptr() if bias is not None else None
        if self.fam == "attention":
            return (H, d, d, SCALE, a, H * d, b, H * d, c, H * d, bp)
        if self.fam == "gat":
            return (H, d, SLOPE, a, H, b, H, c, H * d, bp)
        return (H, d, SLOPE, a, H * d, b, H * d, c, bp)

    def _call(self, suffix, args, drop, plain):
        stream = self.t.cuda.current_stream().cuda_stream
        if plain:
            getattr(self.eng, "%s_%s" % (ENTRY[self.fam], suffix))(*args, stream)
        else:
            getattr(self.eng, "%s_dropout_%s" % (ENTRY[self.fam], suffix))(*args, drop, stream)

    def forward(self, ops, bias, drop, plain=False):
        t, H, d = self.t, self.H, self.d
        O = t.full((self.M, H, d), 7.0, device="cuda"); lse = t.full((self.M, H), 7.0, device="cuda")
        self._call("device", self._lead(ops, bias) + (O.data_ptr(), H * d, lse.data_ptr()), drop, plain)
        return O, lse

    def backward(self, ops, bias, drop, O, lse, G, plain=False):
        """-> delta, [three gradients], dbias (None without bias)"""
        t, H, d, fam = self.t, self.H, self.d, self.fam
        full = lambda *s: t.full(s, 7.0, device="cuda")   # noqa: E731
        delta = full(self.M, H)
        db = full(self.nnz) if bias is not None else None
        dbp = db.data_ptr() if db is not None else None
        tail = (O.data_ptr(), H * d, lse.data_ptr(), G.data_ptr(), H * d, delta.data_ptr())
        if fam == "attention":
            g = [full(self.M, H, d), full(self.K, H, d), full(self.K, H, d)]
            tail += (g[0].data_ptr(), H * d, g[1].data_ptr(), H * d, g[2].data_ptr(), H * d, dbp)
        elif fam == "gat":
            g = [full(self.M, H), full(self.K, H), full(self.K, H, d)]
            tail += (g[0].data_ptr(), H, g[1].data_ptr(), H, g[2].data_ptr(), H * d, dbp)
        else:
            g = [full(self.M, H, d), full(self.K, H, d), full(H, d)]
            self.work = full(self.eng.gatv2_workspace_floats(H, d))
            tail += (g[0].data_ptr(), H * d, g[1].data_ptr(), H * d, g[2].data_ptr(), self.work.data_ptr(), dbp)
        self._call("backward_device", self._lead(ops, bias) + tail, drop, plain)
        return delta, g, db

    def everything(self, ops, bias, drop, G, plain=False):
        """forward and backward -> [O, lse, delta, g0, g1, g2, (dbias)] as numpy"""
        O, lse = self.forward(ops, bias, drop, plain)
        self.fwd_kernel = self.eng.last_kernel()
        delta, g, db = self.backward(ops, bias, drop, O, lse, G, plain)
        self.bwd_kernel = self.eng.last_kernel()
        return [x.cpu().numpy() for x in [O, lse, delta] + g + ([db] if db is not None else [])]


def compare(fam, got, want, rp, has_bias):
    lens = np.diff(rp)
    O, lse, delta = got[:3]
    assert all(np.all(np.isfinite(x)) for x in [O, delta] + got[3:]), fam
    assert _close(O, want["O"]), ("O", float(np.abs(O - want["O"]).max()))
    assert np.all(O[lens == 0].view(np.uint32) == 0) and np.all(lse[lens == 0] == -np.inf)
    assert _close(lse[lens > 0], want["lse"][lens > 0]), "lse"
    assert _close(delta, want["delta"]), ("delta", float(np.abs(delta - want["delta"]).max()))
    for g, w, name in zip(got[3:6], want["grads"], GRADS[fam]):
        assert g.shape == w.shape and _close(g, w), (name, float(np.abs(g - w).max()))
    if has_bias:
        assert _close(got[6], want["dbias"]), ("dbias", float(np.abs(got[6] - want["dbias"]).max()))


def small_pattern(seed):
    """60 x 50, rectangular, with empty rows and with columns that no entry names"""
    rs = np.random.RandomState(seed)
    M, K = 60, 50
    rp, ci, _ = random_csr(rs, M, K - 6, 7, empty_frac=0.15)
    assert np.any(np.diff(rp) == 0) and np.all(np.diff(rp) < 40) and ci.max() < K - 6
    return rs, rp, ci, M, K


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("p", [0.1, 0.6])
@pytest.mark.parametrize("H, d", [(1, 16), (3, 24), (2, 64), (1, 128)])
@pytest.mark.parametrize("fam", FAMILIES)
def test_against_float64_with_the_host_mask(sx, fam, H, d, p, bias):
    import torch
    rs, rp, ci, M, K = small_pattern(11 + d)
    nnz = len(ci)
    bn = rand(rs, nnz) if bias else None
    ops, Gn = operands(fam, rs, M, K, H, d, rp, ci, bn), rand(rs, M, H, d)
    seed, step = 1234567 + d, 3
    mult = host_mult(nnz, H, p, seed, step)
    assert 0 < np.count_nonzero(mult) < mult.size
    step_t = torch.tensor([step], dtype=torch.int64, device="cuda")
    a = Abi(sx, fam, rp, ci, M, K, H, d)
    got = a.everything([torch.from_numpy(x).cuda() for x in ops], torch.from_numpy(bn).cuda() if bias else None,
                       sx.api.Dropout(p, seed, step_t.data_ptr()), torch.from_numpy(Gn).cuda())
    assert a.fwd_kernel == ENTRY[fam].replace("_attention", "") + "_fused+dropout", a.fwd_kernel
    assert a.bwd_kernel == ENTRY[fam].replace("_attention", "") + "_fused_backward+dropout", a.bwd_kernel
    compare(fam, got, reference(fam, rp, ci, M, K, ops, Gn, bn, mult), rp, bias)
    a.eng.close()


def long_pattern(rs):
    """one row of 2049 entries and one column of 2049 entries (both beyond the long-row threshold of 2048), unsymmetric: row 0 holds
    2049 columns; rows 1 .. 2049 hold column 7 and one more column each, so column 7 is a long row of A^T and the position of an entry
    in A^T's arrays differs from its position in A's"""
    K = 2100
    M = 2050
    first = np.sort(rs.choice(np.setdiff1d(np.arange(K), [7]), size=2049, replace=False))
    lens = np.array([2049] + [2] * 2049)
    rp = np.zeros(M + 1, np.int32); rp[1:] = np.cumsum(lens)
    ci = np.zeros(rp[-1], np.int32)
    ci[:2049] = first
    other = rs.randint(8, K, size=2049)
    ci[2049::2] = 7
    ci[2050::2] = other
    return rp, ci, M, K


@pytest.mark.parametrize("fam", FAMILIES)
def test_long_rows_and_the_original_entry_index(sx, fam):
    """The long-row workgroup in the forward and the row pass, the long workgroup in the column pass.  The column pass walks A^T, where
    an entry has another position than in A: only with perm[e] as the hash's counter do dK / dV / dasrc / dx_src agree with the
    reference, whose mask is indexed by A's positions."""
    import torch
    rs = np.random.RandomState(5)
    rp, ci, M, K = long_pattern(rs)
    assert np.diff(rp).max() == 2049 and np.count_nonzero(ci == 7) == 2049
    # the entries of column 7, in A^T's order, are not where they are in A
    order = np.argsort(ci, kind="stable")
    assert np.count_nonzero(order != np.arange(len(ci))) > 2048
    H, d, p, seed = 2, 16, 0.6, 99
    nnz = len(ci)
    bn = rand(rs, nnz)
    ops, Gn = operands(fam, rs, M, K, H, d, rp, ci, bn), rand(rs, M, H, d)
    a = Abi(sx, fam, rp, ci, M, K, H, d)
    got = a.everything([torch.from_numpy(x).cuda() for x in ops], torch.from_numpy(bn).cuda(), sx.api.Dropout(p, seed), torch.from_numpy(Gn).cuda())
    base = ENTRY[fam].replace("_attention", "")
    assert a.fwd_kernel == base + "_fused+dropout+long_rows", a.fwd_kernel
    assert a.bwd_kernel == base + "_fused_backward+dropout+long_rows", a.bwd_kernel
    compare(fam, got, reference(fam, rp, ci, M, K, ops, Gn, bn, host_mult(nnz, H, p, seed)), rp, True)
    a.eng.close()


@pytest.mark.parametrize("fam", FAMILIES)
def test_all_dropped_row(sx, fam):
    """H = 1, seed 7, step 0, p = 0.6 drops the entries 6 .. 14: row 1 is exactly those nine"""
    import torch
    from sextans_amd import api
    keep = api.dropout_keep_host(0, 20, 1, 0.6, 7, 0).ravel()
    assert not keep[6:15].any() and keep[5] and keep[15]
    rs = np.random.RandomState(3)
    M, K, H, d = 3, 24, 1, 16
    rp = np.array([0, 6, 15, 20], np.int32)
    ci = np.concatenate([np.sort(rs.choice(K, size=n, replace=False)) for n in (6, 9, 5)]).astype(np.int32)
    bn = rand(rs, 20)
    ops, Gn = operands(fam, rs, M, K, H, d, rp, ci, bn), rand(rs, M, H, d)
    dev = [torch.from_numpy(x).cuda() for x in ops]
    bias, G = torch.from_numpy(bn).cuda(), torch.from_numpy(Gn).cuda()
    a = Abi(sx, fam, rp, ci, M, K, H, d)
    got = a.everything(dev, bias, sx.api.Dropout(0.6, 7), G)
    plain = a.everything(dev, bias, None, G, plain=True)
    O, lse, delta, g0 = got[:4]
    assert np.all(O[1].view(np.uint32) == 0)                       # +0, the bits
    assert np.all(np.isfinite(lse)) and same(lse, plain[1])        # lse does not see the mask
    assert np.all(delta[1] == 0) and np.all(g0[1] == 0)            # dQ / dadst / dx_dst of the row
    assert np.all(got[6][6:15] == 0)                               # and its dbias
    assert np.any(O[0] != 0) and np.any(g0[0] != 0) and np.any(O[2] != 0)
    compare(fam, got, reference(fam, rp, ci, M, K, ops, Gn, bn, host_mult(20, H, 0.6, 7)), rp, True)
    a.eng.close()


@pytest.mark.parametrize("fam", FAMILIES)
def test_bits(sx, fam):
    import torch
    M, K, H, d = 300, 260, 2, 24
    rs, rp, ci, v = pattern(7, M, K, 9)
    ops, Gn = operands(fam, rs, M, K, H, d, rp, ci, v), rand(rs, M, H, d)
    dev = [torch.from_numpy(x).cuda() for x in ops]
    bias, G = torch.from_numpy(v).cuda(), torch.from_numpy(Gn).cuda()
    a = Abi(sx, fam, rp, ci, M, K, H, d)
    plain = a.everything(dev, bias, None, G, plain=True)
    base = ENTRY[fam].replace("_attention", "")
    assert (a.fwd_kernel, a.bwd_kernel) == (base + "_fused", base + "_fused_backward")
    for drop in (None, sx.api.Dropout(0.0, 0), sx.api.Dropout(0.0, 0xDEADBEEF12345678)):
        got = a.everything(dev, bias, drop, G)
        assert (a.fwd_kernel, a.bwd_kernel) == (base + "_fused", base + "_fused_backward")   # the plain kernels
        assert all(same(x, y) for x, y in zip(got, plain))
    step = torch.tensor([5], dtype=torch.int64, device="cuda")
    one = a.everything(dev, bias, sx.api.Dropout(0.6, 42, step.data_ptr()), G)
    two = a.everything(dev, bias, sx.api.Dropout(0.6, 42, step.data_ptr()), G)
    assert all(same(x, y) for x, y in zip(one, two))
    assert not same(one[0], plain[0]) and same(one[1], plain[1])     # another O, the same lse
    assert all(same(x, y) for x, y in zip(one, a.everything(dev, bias, sx.api.Dropout(0.6, 47), G)))   # seed + step
    other = a.everything(dev, bias, sx.api.Dropout(0.6, 43, step.data_ptr()), G)
    assert not same(one[0], other[0])
    a.eng.close()


def torch_call(fam, A, params, bias=False, **kw):
    from sextans_amd import torch_op
    if fam == "attention":
        return torch_op.sparse_attention_dropout(A, *params, scale=SCALE, bias=bias, fused=True, **kw)
    if fam == "gat":
        return torch_op.gat_attention_dropout(A, *params, negative_slope=SLOPE, bias=bias, **kw)
    return torch_op.gatv2_attention_dropout(A, *params, negative_slope=SLOPE, bias=bias, **kw)


@pytest.mark.parametrize("fam", FAMILIES)
def test_torch_op_against_float64(sx, fam):
    """the autograd Function hands the forward's seed and step to the backward; a bias gradient comes back on A's pattern"""
    import torch
    from sextans_amd import torch_op
    M, K, H, d, p, seed = 300, 260, 3, 24, 0.6, -5          # (a negative int64 seed: its two's complement)
    rs, rp, ci, v = pattern(19, M, K, 9)
    ops, Gn = operands(fam, rs, M, K, H, d, rp, ci, v), rand(rs, M, H, d)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K, grad=True)
    params = [torch.from_numpy(x).cuda().requires_grad_() for x in ops]
    step = torch.tensor(2, dtype=torch.int64, device="cuda")
    out = torch_call(fam, A, params, bias=True, dropout=p, seed=seed, step=step)
    out.backward(torch.from_numpy(Gn).cuda())
    want = reference(fam, rp, ci, M, K, ops, Gn, v, host_mult(len(ci), H, p, seed & M64, 2))
    assert _close(out.detach().cpu().numpy(), want["O"])
    for t, w, name in zip(params, want["grads"], GRADS[fam]):
        assert _close(t.grad.cpu().numpy(), w), name
    assert A.grad.layout == torch.sparse_csr and _close(A.grad.values().cpu().numpy(), want["dbias"])
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            torch_call(fam, A, params, dropout=bad)
    with pytest.raises(TypeError):
        torch_call(fam, A, params, dropout=0.5, seed=1, step=torch.zeros(1, dtype=torch.int32, device="cuda"))
    # dropout = 0 is the op without dropout, bit for bit
    with torch.no_grad():
        zero = torch_call(fam, A, params, bias=True, dropout=0.0, seed=9)
        plain = {"attention": lambda: torch_op.sparse_attention(A, *params, scale=SCALE, bias=True, fused=True),
                 "gat": lambda: torch_op.gat_attention(A, *params, negative_slope=SLOPE, bias=True),
                 "gatv2": lambda: torch_op.gatv2_attention(A, *params, negative_slope=SLOPE, bias=True)}[fam]()
    assert same(zero.cpu().numpy(), plain.cpu().numpy())
    torch_op.clear_cache()


@pytest.mark.parametrize("fam", FAMILIES)
def test_captured_step_draws_a_new_mask_per_replay(sx, fam):
    """forward + backward captured once with `step` as a device tensor; the caller sets it between replays"""
    import torch
    from sextans_amd import torch_op
    M, K, H, d, p, seed = 900, 900, 2, 16, 0.6, 11
    rs, rp, ci, v = pattern(23, M, K, 10)
    ops, Gn = operands(fam, rs, M, K, H, d, rp, ci, None), rand(rs, M, H, d)
    G = torch.from_numpy(Gn).cuda()
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    params = [torch.from_numpy(x).cuda().requires_grad_() for x in ops]
    step = torch.zeros((), dtype=torch.int64, device="cuda")

    def once():
        for t in params:
            t.grad = None
        out = torch_call(fam, A, params, dropout=p, seed=seed, step=step)
        out.backward(G)
        return out

    def state(out):
        return [x.detach().cpu().numpy().copy() for x in [out] + [t.grad for t in params]]

    eager = []
    for k in (0, 1):
        step.fill_(k)
        eager.append(state(once()))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        once()                      # warm-up on the side stream: engine, tables, A^T
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = once()
    assert torch_op.cache_info()["engines_built"] == 1
    replays = []
    for k in (0, 1):
        step.fill_(k)
        g.replay()
        torch.cuda.synchronize()
        replays.append(state(out))
        assert all(same(x, y) for x, y in zip(replays[k], eager[k])), k
    assert not same(replays[0][0], replays[1][0]) and not same(replays[0][1], replays[1][1])
    # step k on the device is seed + k without a step
    with torch.no_grad():
        direct = torch_call(fam, A, params, dropout=p, seed=seed + 1)
    assert same(direct.cpu().numpy(), replays[1][0])
    torch_op.clear_cache()


@pytest.mark.parametrize("heads, p", [(1, 0.1), (3, 0.6), (8, 0.9), (2, 0.0)])
def test_mask_entry_equals_the_host_mask(sx, heads, p):
    import torch
    from sextans_amd import torch_op
    M, K = 300, 260
    rs, rp, ci, v = pattern(29, M, K, 9)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    seed = 0xFEDCBA9876543210
    got = torch_op.dropout_mask(A, heads, p, seed)
    assert got.shape == (len(ci), heads) and got.dtype == torch.float32
    assert same(got.cpu().numpy(), host_mult(len(ci), heads, p, seed))
    step = torch.tensor([7], dtype=torch.uint64, device="cuda")
    assert same(torch_op.dropout_mask(A, heads, p, seed, step).cpu().numpy(), host_mult(len(ci), heads, p, seed, 7))
    # the C entry itself, on its own engine
    rpt, cit = torch.from_numpy(rp.astype(np.int32)).cuda(), torch.from_numpy(ci.astype(np.int32)).cuda()
    eng = sx.Engine(0)
    eng.set_matrix_csr_device(M, K, len(ci), rpt.data_ptr(), cit.data_ptr(), torch.from_numpy(v).cuda().data_ptr())
    out = torch.full((len(ci) * heads + 4,), 7.0, device="cuda")
    eng.dropout_mask_device(heads, sx.api.Dropout(p, seed, step.data_ptr()), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert same(out[:-4].cpu().numpy().reshape(-1, heads), host_mult(len(ci), heads, p, seed, 7)) and bool((out[-4:] == 7.0).all())
    eng.close()
    torch_op.clear_cache()


def test_composition_agrees_with_the_fused_kernels(sx):
    """sparse_attention_dropout(fused=False) multiplies P by the mask entry's column before the SpMM: the same mask as fused=True, so the
    two agree within the tolerance test_fused_attention_gpu.test_agrees_with_the_composition holds them to, gradients included"""
    import torch
    from sextans_amd import torch_op
    M, K, H, d, dv, seed = 500, 420, 3, 16, 32, 77
    rs, rp, ci, v = pattern(41, M, K, 11)
    Qn, Kn, Vn, Gn = rand(rs, M, H, d), rand(rs, K, H, d), rand(rs, K, H, dv), rand(rs, M, H, dv)

    def run(fused, squeeze_head=None):
        torch_op.clear_cache()
        A = make_A(rp, ci, v, M, K, grad=True)
        pick = (lambda t: t) if squeeze_head is None else (lambda t: np.ascontiguousarray(t[:, squeeze_head]))
        Q, Kt, V = (torch.from_numpy(pick(t)).cuda().requires_grad_() for t in (Qn, Kn, Vn))
        out = torch_op.sparse_attention_dropout(A, Q, Kt, V, 0.6, seed=seed, bias=True, fused=fused)
        out.backward(torch.from_numpy(pick(Gn)).cuda())
        return [t.detach().cpu().numpy() for t in (out, Q.grad, Kt.grad, V.grad, A.grad.values())]

    fused, comp = run(True), run(False)
    assert not _close(fused[0], run_plain(rp, ci, v, M, K, Qn, Kn, Vn))     # dropout did something
    for g, w, name in zip(fused, comp, ("O", "dQ", "dK", "dV", "dA")):
        assert _close(g, w), (name, float(np.abs(g - w).max()))
    # one head given as 2-D operands: the mask of heads = 1
    f2, c2 = run(True, 0), run(False, 0)
    for g, w, name in zip(f2, c2, ("O", "dQ", "dK", "dV", "dA")):
        assert _close(g, w), (name, float(np.abs(g - w).max()))
    torch_op.clear_cache()


def run_plain(rp, ci, v, M, K, Qn, Kn, Vn):
    import torch
    from sextans_amd import torch_op
    A = make_A(rp, ci, v, M, K)
    with torch.no_grad():
        return torch_op.sparse_attention(A, *(torch.from_numpy(t).cuda() for t in (Qn, Kn, Vn)), bias=True, fused=True).cpu().numpy()


@pytest.mark.parametrize("fam", FAMILIES)
def test_seed_from_the_default_generator(sx, fam):
    import torch
    from sextans_amd import torch_op
    M, K, H, d = 300, 260, 2, 16
    rs, rp, ci, v = pattern(31, M, K, 9)
    ops = operands(fam, rs, M, K, H, d, rp, ci, None)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    params = [torch.from_numpy(x).cuda() for x in ops]
    with torch.no_grad():
        torch.manual_seed(3)
        first = torch_call(fam, A, params, dropout=0.6).cpu().numpy()
        third = torch_call(fam, A, params, dropout=0.6).cpu().numpy()      # the generator moved on
        torch.manual_seed(3)
        second = torch_call(fam, A, params, dropout=0.6).cpu().numpy()
    assert same(first, second) and not same(first, third)
    torch_op.clear_cache()
