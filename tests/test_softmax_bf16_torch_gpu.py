"""The bf16 edge tensors of the two per-channel softmax families in the torch front end: vector_attention() with bf16 S and D,
spmm_edge_softagg() with a bf16 E, on the 400 x 300 matrix of the reduce tests at N = 728 (nnz N = 2.62 M; twelve tiles, the last one
partial).
  Every comparison is on bits, against the route of the parent commit computed here: the op on the .float() tensors, its gradients cast
with .to(bfloat16) (round to nearest even).  The equivalence the automatic route rests on is asserted, not assumed: for all-bf16
qualifying operands that route returns the bits of the native one -- with special values in the upstream gradient too (NaN, +-inf, -0,
a value that rounds over bf16's range).
  Which kernels ran is read from last_kernel; calls are counted by wrapping the eight Engine methods.
  Peak memory: caps derived from the tensors each route must hold, not from a measurement.  With S = nnz * N elements, above the
operands and G one forward + backward of vector attention in add mode holds, natively, dS + dD in bf16 = 4 S bytes (and tensors of node
size: C, lse, dV and V's gradient, 0.4 S bytes each at most on this matrix), through the fp32 copies at least two fp32 copies and two
fp32 gradients = 16 S: the cap is 8 S.  Edge softagg with a gradient for E: 2 S against 8 S, the cap is 4 S."""
import numpy as np
import pytest

import test_spmm_edge_softagg_gpu as es
import test_vector_attention_gpu as va
from test_edge_bf16_torch_gpu import bf16_of, bits, engine, peak_of, same_bits
from test_fused_attention_gpu import rand
from test_spmm_reduce_gpu import base_matrix
from test_torch_attention_gpu import make_A

pytestmark = pytest.mark.gpu

N = 728
ENTRIES = ("vector_attention_device_rm", "vector_attention_backward_device_rm", "spmm_edge_softagg_device_rm",
           "spmm_edge_softagg_backward_device_rm")
_case = []


def case():
    """the matrix and, as numpy fp32, S (+-4), V, D, E, G (+-1) and the temperatures; once, never changed"""
    if not _case:
        rs, rp, ci, v, M, K = base_matrix(5)
        nnz = len(ci)
        assert nnz * N >= 2_600_000
        _case.append((rp, ci, v, M, K, va.scores(1000 + N, nnz, N), rand(rs, K, N), rand(rs, nnz, N), rand(rs, nnz, N), rand(rs, M, N),
                      es.temps(N)))
    return _case[0]


@pytest.fixture
def calls(monkeypatch):
    """name -> how often the Engine method ran"""
    from sextans_amd import api
    count = {}
    for base in ENTRIES:
        for name in (base, base + "_bf16"):
            def wrapped(self, *a, _f=getattr(api.Engine, name), _n=name, **kw):
                count[_n] = count.get(_n, 0) + 1
                return _f(self, *a, **kw)
            monkeypatch.setattr(api.Engine, name, wrapped)
    return count


def leaf(x, dtype=None):
    """numpy or tensor -> a fresh CUDA leaf that requires grad (None stays None)"""
    import torch
    if x is None:
        return None
    t = torch.from_numpy(x).cuda() if isinstance(x, np.ndarray) else x.detach().clone()
    return (t if dtype is None else t.to(dtype)).requires_grad_()


# --- vector attention ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["node", "add", "edge"])
def test_vector_attention_takes_the_bf16_kernels_and_returns_the_bits_of_the_route_through_fp32(sx, calls, mode):
    import torch
    from sextans_amd import torch_op
    from sextans_amd.vector_attention import vector_attention
    rp, ci, v, M, K, S, V, D, _, G, _ = case()
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    S16, D16, Gt = bf16_of(S), bf16_of(D), torch.from_numpy(G).cuda()
    Vn, Dn = (V if mode != "edge" else None), (D16 if mode != "node" else None)
    # the route of the parent commit: the fp32 op on the .float() tensors, the gradients cast to the operands' dtype
    rS, rV, rD = leaf(S16, torch.float32), leaf(Vn), leaf(Dn, torch.float32)
    rC, rL = vector_attention(A, rS, rV, rD, return_lse=True)
    assert engine().last_kernel() == "vector_attention"
    rC.backward(Gt)
    assert engine().last_kernel() == "vector_attention_backward"
    assert calls == {"vector_attention_device_rm": 1, "vector_attention_backward_device_rm": 1}, calls
    calls.clear()
    # all edge tensors bf16 and qualifying: the native route
    St, Vt, Dt = leaf(S16), leaf(Vn), leaf(Dn)
    C, L = vector_attention(A, St, Vt, Dt, return_lse=True)
    assert engine().last_kernel() == "vector_attention_bf16"
    assert C.dtype == torch.float32 and L.dtype == torch.float32 and same_bits(C, rC) and same_bits(L, rL), mode
    C.backward(Gt)
    assert engine().last_kernel() == "vector_attention_backward_bf16"
    assert calls == {"vector_attention_device_rm_bf16": 1, "vector_attention_backward_device_rm_bf16": 1}, calls
    assert St.grad.dtype == torch.bfloat16 and same_bits(St.grad, rS.grad.to(torch.bfloat16)), mode
    if Dt is not None:
        assert Dt.grad.dtype == torch.bfloat16 and same_bits(Dt.grad, rD.grad.to(torch.bfloat16)), mode
    if Vt is not None:
        assert Vt.grad.dtype == torch.float32 and same_bits(Vt.grad, rV.grad), mode
    # without autograd: the same bits, one more forward call
    with torch.no_grad():
        assert same_bits(vector_attention(A, St, Vt, Dt), C)
    assert calls["vector_attention_device_rm_bf16"] == 2 and engine().last_kernel() == "vector_attention_bf16"
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0 and info["entries"] == 1, info
    torch_op.clear_cache()


def test_vector_attention_other_calls_keep_the_fp32_kernels(sx, calls):
    """a mixed call, an N that is no multiple of 8 and a bf16 tensor that is not row-major take the fp32 copies, as before, and are no
    errors; trailing shapes and node operands in another dtype work on the native route"""
    import torch
    from sextans_amd import torch_op
    from sextans_amd.vector_attention import vector_attention
    rp, ci, v, M, K, S, V, D, _, G, _ = case()
    nnz = len(ci)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    S16, D16, Vt, Gt = bf16_of(S), bf16_of(D), torch.from_numpy(V).cuda(), torch.from_numpy(G).cuda()
    want = vector_attention(A, S16.float(), Vt, D16.float())
    for s, d in ((S16, D16.float()), (S16.float(), D16), (S16.t().contiguous().t(), D16)):   # mixed, mixed, a column-major S
        s, d = s.detach().requires_grad_(), d.detach().requires_grad_()
        C = vector_attention(A, s, Vt, d)
        assert engine().last_kernel() == "vector_attention" and same_bits(C, want)
        C.backward(Gt)
        assert engine().last_kernel() == "vector_attention_backward" and s.grad.dtype == s.dtype and d.grad.dtype == d.dtype
    n5 = 13                                                                                # N % 8 != 0: padded fp32 copies
    s5, d5 = S16[:, :n5].clone().requires_grad_(), D16[:, :n5].clone().requires_grad_()
    C5 = vector_attention(A, s5, Vt[:, :n5], d5)
    assert engine().last_kernel() == "vector_attention" and same_bits(C5, vector_attention(A, s5.detach().float(), Vt[:, :n5], d5.detach().float()))
    C5.backward(Gt[:, :n5])
    assert engine().last_kernel() == "vector_attention_backward" and s5.grad.dtype == torch.bfloat16 and d5.grad.shape == (nnz, n5)
    assert not any(k.endswith("_bf16") for k in calls), calls
    # a trailing shape on the native route: (nnz, 91, 8)
    s3, d3, v3 = leaf(S16.reshape(nnz, 91, 8)), leaf(D16.reshape(nnz, 91, 8)), leaf(Vt.reshape(K, 91, 8))
    C3, L3 = vector_attention(A, s3, v3, d3, return_lse=True)
    assert engine().last_kernel() == "vector_attention_bf16" and C3.shape == (M, 91, 8) and L3.shape == (M, 91, 8)
    assert same_bits(C3.reshape(M, N), want)
    C3.backward(Gt.reshape(M, 91, 8))
    assert engine().last_kernel() == "vector_attention_backward_bf16"
    s2, d2, v2 = leaf(S16, torch.float32), leaf(D16, torch.float32), leaf(Vt)
    vector_attention(A, s2, v2, d2).backward(Gt)
    assert s3.grad.shape == s3.shape and s3.grad.dtype == torch.bfloat16 and same_bits(s3.grad.reshape(nnz, N), s2.grad.to(torch.bfloat16))
    assert same_bits(d3.grad.reshape(nnz, N), d2.grad.to(torch.bfloat16)) and same_bits(v3.grad.reshape(K, N), v2.grad)
    # a node operand in another dtype is widened by torch as before; its gradient comes back in that dtype
    vh = leaf(Vt, torch.bfloat16)
    Ch = vector_attention(A, leaf(S16), vh, leaf(D16))
    assert engine().last_kernel() == "vector_attention_bf16" and Ch.dtype == torch.float32
    assert same_bits(Ch, vector_attention(A, S16.float(), vh.detach().float(), D16.float()))
    Ch.backward(Gt)
    assert vh.grad.dtype == torch.bfloat16
    torch_op.clear_cache()


# --- edge softagg ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["mul", "add", "add_relu", "copy"])
def test_edge_softagg_takes_the_bf16_kernels_and_returns_the_bits_of_the_route_through_fp32(sx, calls, op):
    import torch
    from sextans_amd import torch_op
    from sextans_amd.edge_softagg import spmm_edge_softagg
    rp, ci, v, M, K, _, B, _, E, G, t = case()
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    E16, Gt = bf16_of(E), torch.from_numpy(G).cuda()
    Bn = B if op != "copy" else None
    rB, rE, rt = leaf(Bn), leaf(E16, torch.float32), leaf(t)
    rC, rL = spmm_edge_softagg(A, rB, rE, op=op, t=rt, return_lse=True)
    assert engine().last_kernel() == "spmm_edge_softagg"
    rC.backward(Gt)
    assert engine().last_kernel() == "spmm_edge_softagg_backward"
    assert calls == {"spmm_edge_softagg_device_rm": 1, "spmm_edge_softagg_backward_device_rm": 1}, calls
    calls.clear()
    Bt, Et, tt = leaf(Bn), leaf(E16), leaf(t)
    C, L = spmm_edge_softagg(A, Bt, Et, op=op, t=tt, return_lse=True)
    assert engine().last_kernel() == "spmm_edge_softagg_bf16"
    assert C.dtype == torch.float32 and L.dtype == torch.float32 and same_bits(C, rC) and same_bits(L, rL), op
    C.backward(Gt)
    assert engine().last_kernel() == "spmm_edge_softagg_backward_bf16"
    assert calls == {"spmm_edge_softagg_device_rm_bf16": 1, "spmm_edge_softagg_backward_device_rm_bf16": 1}, calls
    assert Et.grad.dtype == torch.bfloat16 and same_bits(Et.grad, rE.grad.to(torch.bfloat16)), op
    assert tt.grad.dtype == torch.float32 and same_bits(tt.grad, rt.grad), op
    if Bt is not None:
        assert Bt.grad.dtype == torch.float32 and same_bits(Bt.grad, rB.grad), op
    with torch.no_grad():   # without autograd, t = 1 (the kernels' t == NULL path), eps
        assert same_bits(spmm_edge_softagg(A, Bt, Et, op=op, eps=0.5), spmm_edge_softagg(A, rB, rE, op=op, eps=0.5))
    assert engine().last_kernel() == "spmm_edge_softagg"      # (the last call above: the fp32 one)
    assert calls["spmm_edge_softagg_device_rm_bf16"] == 2
    # a bf16 E the kernel cannot read where it lies keeps the fp32 kernel: N % 8 != 0, and a column-major E
    for e in (E16[:, :13].clone(), E16.t().contiguous().t()):
        e.requires_grad_()
        b = Bt.detach()[:, :e.shape[1]] if Bt is not None else None
        Ce = spmm_edge_softagg(A, b, e, op=op)
        assert engine().last_kernel() == "spmm_edge_softagg"
        Ce.backward(Gt[:, :e.shape[1]])
        assert engine().last_kernel() == "spmm_edge_softagg_backward" and e.grad.dtype == torch.bfloat16
    assert calls["spmm_edge_softagg_device_rm_bf16"] == 2 and calls["spmm_edge_softagg_backward_device_rm_bf16"] == 1
    info = torch_op.cache_info()
    assert info["engines_built"] == 1 and info["value_refreshes"] == 0 and info["entries"] == 1, info
    torch_op.clear_cache()


# --- the equivalence with special values in the upstream gradient ----------------------------------------------------------------------------
def test_special_values_of_G_come_back_as_the_route_through_fp32_returns_them(sx):
    """NaN, +-inf, -0 and 0x7F7FC000 (finite in fp32, inf in bf16) in G, each in a row and column of its own: the native route's bf16
    gradients have the bits of the fp32 gradients cast by torch"""
    import torch
    from sextans_amd import torch_op
    from sextans_amd.edge_softagg import spmm_edge_softagg
    from sextans_amd.vector_attention import vector_attention
    rp, ci, v, M, K, S, V, D, E, G, t = case()
    rows = np.flatnonzero(np.diff(rp) > 1)[[3, 40, 80, 120, 160]]
    G2 = G.copy()
    G2[rows, [5, 100, 333, 600, 727]] = np.array([0x7FC00000, 0x7F800000, 0xFF800000, 0x80000000, 0x7F7FC000], np.uint32).view(np.float32)
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    S16, D16, E16, Gt = bf16_of(S), bf16_of(D), bf16_of(E), torch.from_numpy(G2).cuda()
    rS, rV, rD = leaf(S16, torch.float32), leaf(V), leaf(D16, torch.float32)
    vector_attention(A, rS, rV, rD).backward(Gt)
    St, Vt, Dt = leaf(S16), leaf(V), leaf(D16)
    vector_attention(A, St, Vt, Dt).backward(Gt)
    assert engine().last_kernel() == "vector_attention_backward_bf16"
    for name, g, r in (("dS", St.grad, rS.grad), ("dD", Dt.grad, rD.grad)):
        w = r.to(torch.bfloat16)
        print("vector_attention", name, "non-finite:", int((~torch.isfinite(g.float())).sum()), "NaN:", int(torch.isnan(g.float()).sum()),
              "bit patterns that differ:", int((bits(g) != bits(w)).sum()))
        assert same_bits(g, w), name
    assert int(torch.isnan(Dt.grad.float()).sum()) > 0 and int(torch.isinf(Dt.grad.float()).sum()) > 0   # (the values arrived)
    assert same_bits(Vt.grad, rV.grad)
    for op in ("add_relu", "copy"):
        rB, rE = leaf(V if op != "copy" else None), leaf(E16, torch.float32)
        spmm_edge_softagg(A, rB, rE, op=op, t=torch.from_numpy(t).cuda()).backward(Gt)
        Bt, Et = leaf(V if op != "copy" else None), leaf(E16)
        spmm_edge_softagg(A, Bt, Et, op=op, t=torch.from_numpy(t).cuda()).backward(Gt)
        assert engine().last_kernel() == "spmm_edge_softagg_backward_bf16"
        w = rE.grad.to(torch.bfloat16)
        print("spmm_edge_softagg", op, "dE non-finite:", int((~torch.isfinite(Et.grad.float())).sum()), "NaN:",
              int(torch.isnan(Et.grad.float()).sum()), "bit patterns that differ:", int((bits(Et.grad) != bits(w)).sum()))
        assert same_bits(Et.grad, w), op
        if Bt is not None:
            assert same_bits(Bt.grad, rB.grad), op
    torch_op.clear_cache()


# --- peak memory -----------------------------------------------------------------------------------------------------------------------------
def test_peak_memory_of_forward_and_backward(sx):
    import torch
    from sextans_amd import torch_op
    from sextans_amd.edge_softagg import spmm_edge_softagg
    from sextans_amd.vector_attention import vector_attention
    rp, ci, v, M, K, S, V, D, E, G, _ = case()
    S_el = len(ci) * N
    torch_op.clear_cache()
    A = make_A(rp, ci, v, M, K)
    S16, D16, E16, Vt, Gt = bf16_of(S), bf16_of(D), bf16_of(E), torch.from_numpy(V).cuda(), torch.from_numpy(G).cuda()
    s, d, e, vv = (x.requires_grad_() for x in (S16, D16, E16, Vt))

    def clear():
        for x in (s, d, e, vv):
            x.grad = None

    def vatt(s_, d_):
        vector_attention(A, s_, vv, d_).backward(Gt)

    def soft(e_):
        spmm_edge_softagg(A, Vt.detach(), e_, op="add_relu").backward(Gt)

    # what the parent commit does with bf16 operands: the mixed call below takes the same fp32 copies, D's own copy made outside
    d32 = D16.detach().float().requires_grad_()
    for native, copies, cap, what in ((lambda: vatt(s, d), lambda: vatt(s, d32), 8 * S_el, "vector_attention add"),
                                      (lambda: soft(e), None, 4 * S_el, "spmm_edge_softagg add_relu")):
        native(), clear()                 # (the engine, A^T and torch's own one-time allocations)
        p16 = peak_of(native)
        clear()
        print(what, "peak bytes above the operands and G, native route:", p16, "= %.2f S; cap %.0f S" % (p16 / S_el, cap / S_el))
        if copies is not None:
            copies(), clear()
            d32.grad = None
            p32 = peak_of(copies)
            clear()
            d32.grad = None
            print(what, "through fp32 copies (D already fp32):", p32, "= %.2f S" % (p32 / S_el))
        assert p16 < cap, what
    torch_op.clear_cache()
