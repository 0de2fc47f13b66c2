"""torch_op.spmm with bf16 dense operands: a qualifying bf16 B goes to the bf16 entry point as it lies (no fp32 copy), the default result
keeps the bits of spmm(A, B.float()), out_dtype=torch.bfloat16 returns their rounding, and a bf16 upstream gradient gives dB in bf16."""
import numpy as np
import pytest

from util import random_csr

pytestmark = pytest.mark.gpu


def _bits(t):
    """every NaN made the same NaN, then the raw bits"""
    import torch
    t = torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t).contiguous().cpu()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _round(t32):
    """torch's CPU rounding of an fp32 tensor"""
    return t32.cpu().to(__import__("torch").bfloat16).cuda()


def _matrix(kind, seed=4):
    import torch
    from sextans_amd import api
    rs = np.random.RandomState(seed)
    if kind == "gather":                      # no B-row reuse: the native bf16 route
        M, K = 6000, 5000
        rp, ci, v = random_csr(rs, M, K, 11, long_rows=1)
    else:                                     # LDS-panel plan: the converting route
        rp, ci, v = api.gen_fem3d_host(14, 13, 12, 3, 7)
        M = K = 14 * 13 * 12 * 3
    A = torch.sparse_csr_tensor(torch.from_numpy(rp.astype(np.int64)), torch.from_numpy(ci.astype(np.int64)), torch.from_numpy(v),
                                size=(M, K)).cuda()
    return A, M, K


def _engine(torch_op):
    return next(iter(torch_op._cache.values()))[0]


@pytest.mark.parametrize("kind", ["gather", "fem"])
@pytest.mark.parametrize("transpose_a", [False, True])
def test_bf16_b_forward(sx, kind, transpose_a):
    import torch
    from sextans_amd import torch_op
    A, M, K = _matrix(kind)
    rows_b, rows_c = (M, K) if transpose_a else (K, M)
    g = torch.Generator().manual_seed(1)
    for N in (32, 40):
        B = (torch.rand((rows_b, N), generator=g) * 2 - 1).to(torch.bfloat16).cuda()
        C = (torch.rand((rows_c, N), generator=g) * 2 - 1).cuda()
        torch_op.clear_cache()
        ref = torch_op.spmm(A, B.float(), 0.85, -2.06, C, transpose_a=transpose_a)              # today's fp32 call on the widened B
        info = torch_op.cache_info()
        eng = _engine(torch_op)
        assert (eng.get_stat("bf16_native_calls"), eng.get_stat("bf16_converted_calls")) == (0, 0)
        got = torch_op.spmm(A, B, 0.85, -2.06, C, transpose_a=transpose_a)
        assert got.dtype == torch.float32 and _same(got, ref)
        assert torch_op.cache_info() == info                                                   # same engine, nothing rebuilt or refreshed
        n, c = eng.get_stat("bf16_native_calls"), eng.get_stat("bf16_converted_calls")
        assert (n, c) == ((1, 0) if kind == "gather" else (0, 1)), (n, c, eng.last_kernel())    # B went to the bf16 entry as it lies
        # bf16 result: the rounding of the fp32 result; C given in bf16 is widened exactly
        C16 = C.to(torch.bfloat16)
        ref16 = torch_op.spmm(A, B.float(), 0.85, -2.06, C16.float(), transpose_a=transpose_a)
        got16 = torch_op.spmm(A, B, 0.85, -2.06, C16, transpose_a=transpose_a, out_dtype=torch.bfloat16)
        assert got16.dtype == torch.bfloat16 and _same(got16, _round(ref16))
        assert _same(C16, C.to(torch.bfloat16))                                                 # C untouched
        out = torch.empty((rows_c, N), dtype=torch.bfloat16, device="cuda")
        assert torch_op.spmm(A, B, 0.85, -2.06, C16, out=out, transpose_a=transpose_a, out_dtype=torch.bfloat16) is out and _same(out, got16)
        inplace = C16.clone()
        torch_op.spmm(A, B, 0.85, -2.06, inplace, out=inplace, transpose_a=transpose_a, out_dtype=torch.bfloat16)
        assert _same(inplace, got16)
        # an fp32 C with a bf16 B and a bf16 result: C is NOT rounded before the product -- the fp32 result is rounded once
        assert _same(torch_op.spmm(A, B, 0.85, -2.06, C, transpose_a=transpose_a, out_dtype=torch.bfloat16), _round(ref))
        out = torch.empty((rows_c, N), dtype=torch.bfloat16, device="cuda")
        assert torch_op.spmm(A, B, 0.85, -2.06, C, out=out, transpose_a=transpose_a, out_dtype=torch.bfloat16) is out and _same(out, _round(ref))
        # ... and a bf16 C with the default fp32 result is widened exactly
        assert _same(torch_op.spmm(A, B, 0.85, -2.06, C16, transpose_a=transpose_a), ref16)
        # no C: zeros; fp32 B with out_dtype=bf16: the fp32 call and one rounding pass
        assert _same(torch_op.spmm(A, B, out_dtype=torch.bfloat16, transpose_a=transpose_a),
                     _round(torch_op.spmm(A, B.float(), transpose_a=transpose_a)))
        assert _same(torch_op.spmm(A, B.float(), 0.85, -2.06, C, transpose_a=transpose_a, out_dtype=torch.bfloat16), _round(ref))
        out = torch.empty((rows_c, N), dtype=torch.bfloat16, device="cuda")
        assert torch_op.spmm(A, B.float(), 0.85, -2.06, C, out=out, transpose_a=transpose_a, out_dtype=torch.bfloat16) is out and _same(out, _round(ref))
        with pytest.raises(ValueError):
            torch_op.spmm(A, B, out=torch.empty((rows_c, N), device="cuda"), out_dtype=torch.bfloat16)      # out of the wrong dtype
        with pytest.raises(TypeError):
            torch_op.spmm(A, B, out_dtype=torch.float16)
    torch_op.clear_cache()


def test_bf16_b_that_does_not_qualify_keeps_todays_path(sx):
    """N = 20 (padded to 24), a row stride that is not a multiple of 8, a base 2 bytes off: through the padded fp32 copy, same bits."""
    import torch
    from sextans_amd import torch_op
    A, M, K = _matrix("gather")
    g = torch.Generator().manual_seed(2)
    torch_op.clear_cache()
    B20 = (torch.rand((K, 20), generator=g) * 2 - 1).to(torch.bfloat16).cuda()
    wide = (torch.rand((K, 36), generator=g) * 2 - 1).to(torch.bfloat16).cuda()
    flat = (torch.rand((K * 32 + 1,), generator=g) * 2 - 1).to(torch.bfloat16).cuda()
    C32 = (torch.rand((M, 32), generator=g) * 2 - 1).cuda()
    for B in (B20, wide[:, :32], flat[1:].view(K, 32)):
        got = torch_op.spmm(A, B)
        assert got.dtype == torch.float32 and got.shape == (M, B.shape[1]) and _same(got, torch_op.spmm(A, B.float()))
        assert _same(torch_op.spmm(A, B, out_dtype=torch.bfloat16), _round(got))
        # with an fp32 C the bits do not depend on whether B can be read in place: one rounding, of the result
        assert _same(torch_op.spmm(A, B, 0.85, -2.06, C32[:, :B.shape[1]], out_dtype=torch.bfloat16),
                     _round(torch_op.spmm(A, B.float(), 0.85, -2.06, C32[:, :B.shape[1]])))
    eng = _engine(torch_op)
    assert (eng.get_stat("bf16_native_calls"), eng.get_stat("bf16_converted_calls")) == (0, 0)
    # a padded row stride that does qualify (40 = 5 * 8 elements) is read in place
    B = wide.new_zeros((K, 40))[:, :32].copy_(wide[:, :32])
    assert B.stride(0) == 40 and _same(torch_op.spmm(A, B), torch_op.spmm(A, B.float()))
    assert eng.get_stat("bf16_native_calls") == 1
    assert _same(torch_op.spmm(A, B, 0.85, -2.06, C32, out_dtype=torch.bfloat16), _round(torch_op.spmm(A, B.float(), 0.85, -2.06, C32)))
    assert eng.get_stat("bf16_native_calls") == 2                       # (still read in place: fp32 C on the bf16 entry)
    torch_op.clear_cache()


def test_the_fp32_copy_of_b_is_gone(sx):
    """Allocations, not time: one warm call with a qualifying bf16 B allocates less often than the same call forced through B.float()."""
    import torch
    from sextans_amd import torch_op
    A, M, K = _matrix("gather")
    B = (torch.rand((K, 64)) * 2 - 1).to(torch.bfloat16).cuda()
    torch_op.clear_cache()
    torch_op.spmm(A, B); torch_op.spmm(A, B.float())            # warm: engine, plans
    torch.cuda.synchronize()

    def allocations(f):
        before = torch.cuda.memory_stats()["allocation.all.allocated"]
        r = f()
        torch.cuda.synchronize()
        n = torch.cuda.memory_stats()["allocation.all.allocated"] - before
        del r
        return n

    direct = allocations(lambda: torch_op.spmm(A, B))
    copied = allocations(lambda: torch_op.spmm(A, B.float()))
    assert direct < copied, (direct, copied)
    assert direct == 1, direct                                  # the result tensor, nothing else
    torch_op.clear_cache()


@pytest.mark.parametrize("kind", ["gather", "fem"])
@pytest.mark.parametrize("transpose_a", [False, True])
def test_bf16_gradients(sx, kind, transpose_a):
    """bf16 B requiring grad, bf16 upstream gradient: dB is bf16 and is the rounding of the fp32 backward on the widened inputs; dA keeps
    going through the fp32 SDDMM, with the same bits; with the default fp32 result dB still comes back in B's dtype."""
    import torch
    from sextans_amd import torch_op
    A, M, K = _matrix(kind)
    rows_b, rows_c = (M, K) if transpose_a else (K, M)
    g = torch.Generator().manual_seed(3)
    N = 32
    B16 = (torch.rand((rows_b, N), generator=g) * 2 - 1).to(torch.bfloat16).cuda()
    G16 = (torch.rand((rows_c, N), generator=g) * 2 - 1).to(torch.bfloat16).cuda()
    torch_op.clear_cache()
    B32 = B16.float().requires_grad_(True)
    Ag = A.requires_grad_()
    torch_op.spmm(Ag, B32, 0.85, transpose_a=transpose_a).backward(G16.float())             # the fp32 backward on the widened inputs
    dA_ref = Ag.grad.values().clone()
    Ag.grad = None
    Bb = B16.clone().requires_grad_(True)
    out = torch_op.spmm(Ag, Bb, 0.85, transpose_a=transpose_a, out_dtype=torch.bfloat16)
    assert out.dtype == torch.bfloat16
    out.backward(G16)
    assert Bb.grad.dtype == torch.bfloat16 and _same(Bb.grad, _round(B32.grad))
    assert _same(Ag.grad.values(), dA_ref)
    engines = [ent[0] for ent in torch_op._cache.values()]
    moved = [(e.get_stat("bf16_native_calls"), e.get_stat("bf16_converted_calls")) for e in engines]
    assert sum(n + c for n, c in moved) == 2, moved                                            # forward and dB, both on the bf16 entry
    assert all((c == 0) if kind == "gather" else (n == 0) for n, c in moved), moved
    # default out_dtype: an fp32 result, whose upstream gradient autograd delivers in fp32 -- dB comes back in B's dtype as before
    Bc = B16.clone().requires_grad_(True)
    out = torch_op.spmm(A, Bc, 0.85, transpose_a=transpose_a)
    assert out.dtype == torch.float32
    out.backward(G16.float())
    assert Bc.grad.dtype == torch.bfloat16 and _same(Bc.grad, _round(B32.grad))
    torch_op.clear_cache()
