"""Seed discipline of the five dropout-capable attention calls: without dropout no seed is drawn -- torch's default CPU generator does
not move -- and the result has the bits of the plain call; with dropout and seed=None exactly the generator moves, with a given seed it
does not.  One tiny pattern (40 x 32, about 6 entries per row), H = 2, d = dv = 8."""
import numpy as np
import pytest

from test_fused_attention_gpu import rand, same
from test_torch_attention_gpu import make_A, pattern

gpu = pytest.mark.gpu

M, K, H, D = 40, 32, 2, 8
CALLS = ["sparse_attention_dropout", "sparse_attention_edge", "gat_attention_dropout", "gatv2_attention_dropout", "score_attention"]

_shared = {}


def inputs():
    """the pattern and every operand, made once"""
    if not _shared:
        import torch
        rs, rp, ci, v = pattern(40, M, K, 6)
        nnz = len(ci)
        _shared["A"] = make_A(rp, ci, v, M, K)
        for name, shape in (("Q", (M, H, D)), ("K", (K, H, D)), ("V", (K, H, D)), ("Ek", (nnz, H, D)), ("Ev", (nnz, H, D)), ("ad", (M, H)),
                            ("as", (K, H)), ("xd", (M, H, D)), ("xs", (K, H, D)), ("att", (H, D)), ("S", (nnz, H))):
            _shared[name] = torch.from_numpy(rand(rs, *shape)).cuda()
    return _shared


def call(name, t, **drop):
    """the call with dropout arguments, or (none given) the plain call it must equal at dropout=0"""
    from sextans_amd import torch_op
    A = t["A"]
    if name == "sparse_attention_dropout":
        return torch_op.sparse_attention_dropout(A, t["Q"], t["K"], t["V"], fused=True, **drop) if drop else \
            torch_op.sparse_attention(A, t["Q"], t["K"], t["V"], fused=True)
    if name == "sparse_attention_edge":
        return torch_op.sparse_attention_edge(A, t["Q"], t["K"], t["V"], t["Ek"], t["Ev"], **drop)
    if name == "gat_attention_dropout":
        return torch_op.gat_attention_dropout(A, t["ad"], t["as"], t["V"], **drop) if drop else torch_op.gat_attention(A, t["ad"], t["as"], t["V"])
    if name == "gatv2_attention_dropout":
        return torch_op.gatv2_attention_dropout(A, t["xd"], t["xs"], t["att"], **drop) if drop else \
            torch_op.gatv2_attention(A, t["xd"], t["xs"], t["att"])
    return torch_op.score_attention(A, t["S"], t["V"], **drop)


@gpu
@pytest.mark.parametrize("name", CALLS)
def test_the_generator_moves_only_for_a_drawn_seed(sx, name):
    import torch
    from sextans_amd import torch_op
    t = inputs()
    with torch.no_grad():
        plain = call(name, t).cpu().numpy()
        before = torch.get_rng_state()
        zero = call(name, t, dropout=0.0).cpu().numpy()
        assert torch.equal(torch.get_rng_state(), before)          # dropout=0: no seed drawn
        assert same(zero, plain)                                   # ... and the plain call's bits
        call(name, t, dropout=0.5, seed=7)
        assert torch.equal(torch.get_rng_state(), before)          # a given seed: nothing drawn
        call(name, t, dropout=0.5, seed=None)
        assert not torch.equal(torch.get_rng_state(), before)      # seed=None: drawn from the default generator
    torch.cuda.synchronize()
    torch_op.clear_cache()
