"""The channel-wise attention from per-channel scores (sextans_vector_attention_device_rm / _backward_device_rm) on every row-dealing path
of pattern_pass.h: the 92-row pattern P of test_pattern_dealing_gpu.py (one slot group per row, several slots per row, an idle slot
group, the second walk, the long-row kernel, empty rows) and its transpose P^T, whose column pass walks P with P's own tables -- the
long-row kernel on A and on A^T, asserted through last_kernel.  Every slot width of the family: N = 8, 16, 32, 64.
  Two checks per (pattern, N): all three modes against the float64 reference of test_vector_attention_gpu.py, forward and the gradients,
under its tolerance (_close, rtol 2e-4) with the operands of operands(); and the sharper forward check of test_pattern_dealing_gpu.py --
S = 0 and non-zero integer messages, so that every weight is exactly 1 / n and C the exact integer sum over n (mean_is_exact): a lost,
doubled or misplaced entry shows.
  The fp32 emulation of test_vector_attention_gpu.py on P with these operands, a long row dealt to 8 partial states
(tests/test_vector_attention_tolerance.py), reaches error / limit
    node 0.036 (dS)    add 0.011 (dS)    edge 0.006 (dS)        (C <= 0.007, lse <= 0.001, dV <= 0.004, dD <= 0.002 everywhere)
-- below 0.5: the operands are used as they are."""
import numpy as np
import pytest

import test_vector_attention_gpu as va
from test_fused_attention_gpu import rand
from test_pattern_dealing_gpu import empty_rows_ok, int_values, mean_is_exact, pat, rng

pytestmark = pytest.mark.gpu

WIDTHS = [8, 16, 32, 64]
PATTERNS = ["P", "PT"]


def operands(rs, p, N):
    """S uniform in +-4, V and D in +-1/2 (the scale test_edge_softagg_dealing_gpu.operands settled on for P's rows of 2000 and more
    entries), G in +-1"""
    half = np.float32(0.5)
    return rand(rs, p.nnz, N) * np.float32(4), rand(rs, p.K, N) * half, rand(rs, p.nnz, N) * half, rand(rs, p.M, N)


def names_ok(p, mode, fwd, bwd):
    """every pass over P runs the long-row kernel: the forward and the row pass on P, the column pass (there is none for edge) on P^T"""
    assert fwd == "vector_attention" + ("+long_rows" if p.long_rows else ""), fwd
    assert bwd == "vector_attention_backward" + ("+long_rows" if p.long_rows or mode != "edge" else ""), bwd


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("N", WIDTHS)
def test_vector_attention(sx, N, name):
    p = pat(name)
    a = va.VattAbi(sx, p.rp, p.ci, np.ones(p.nnz, np.float32), p.M, p.K)
    for mode in va.MODES:
        S, V, D, G = operands(rng("vector_attention", mode, N, name), p, N)
        names = va.grads_of(mode)
        C, lse, _, _ = a.fwd(mode, S, V, D)
        fwd = a.eng.last_kernel()
        got = a.bwd(mode, S, V, D, C, lse, G, want=names)
        names_ok(p, mode, fwd, a.eng.last_kernel())
        if "dV" in names:   # the row pass alone: +long_rows on P only
            a.bwd(mode, S, V, D, C, lse, G, want=("dS",))
            assert a.eng.last_kernel() == "vector_attention_backward" + ("+long_rows" if p.long_rows else "")
        va.check(mode, (C, lse), got, va.reference(mode, p.rp, p.ci, S, V, D, G, p.K), "%s N=%d" % (name, N))
        empty_rows_ok(p, C, lse)
    a.eng.close()


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("N", WIDTHS)
def test_uniform_scores_vector_attention(sx, N, name):
    """S = 0: the weights are 1 / n.  node: int_values; add: +-3 / +-4 plus +-1, an integer of magnitude 2 .. 5; edge: int_values"""
    p, rs = pat(name), rng("u-vector_attention", N, name)
    sign = lambda *shape: rs.choice([-1, 1], shape).astype(np.float32)   # noqa: E731
    cases = {"node": (int_values(rs, p.K, N), None),
             "add": ((rs.randint(3, 5, (p.K, N)) * sign(p.K, N)).astype(np.float32), sign(p.nnz, N)),
             "edge": (None, int_values(rs, p.nnz, N))}
    S = np.zeros((p.nnz, N), np.float32)
    a = va.VattAbi(sx, p.rp, p.ci, np.ones(p.nnz, np.float32), p.M, p.K)
    for mode, (V, D) in cases.items():
        C, lse, _, _ = a.fwd(mode, S, V, D)
        assert a.eng.last_kernel() == "vector_attention" + ("+long_rows" if p.long_rows else "")
        mean_is_exact(p, C, lse, va.messages32(mode, V, D, p.ci))
    a.eng.close()
