"""The edge-feature softmax aggregation (sextans_spmm_edge_softagg_device_rm / _backward_device_rm) on every row-dealing path of
pattern_pass.h: the 92-row pattern P of test_pattern_dealing_gpu.py (one slot group per row, several slots per row, an idle slot group,
the second walk, the long-row kernel, empty rows) and its transpose P^T, whose column pass walks P with P's own tables -- the long-row
kernel on A and on A^T, asserted through last_kernel.  Every slot width of the family: N = 8, 16, 32, 64.
  Two checks per (pattern, N): all four ops against the float64 reference of test_spmm_edge_softagg_gpu.py, forward and the three
gradients, under its tolerance (_close, rtol 2e-4) with B and E uniform in +-1/2 (operands() says why); and the sharper forward check of test_pattern_dealing_gpu.py -- t = 0 and non-zero integer messages, so
that every weight is exactly 1 / n and C the exact integer sum over n (mean_is_exact): a lost, doubled or misplaced entry shows."""
import numpy as np
import pytest

import test_spmm_edge_softagg_gpu as es
from test_fused_attention_gpu import rand
from test_pattern_dealing_gpu import empty_rows_ok, int_values, mean_is_exact, pat, rng
from test_torch_autograd_gpu import _close

pytestmark = pytest.mark.gpu

WIDTHS = [8, 16, 32, 64]
PATTERNS = ["P", "PT"]


def operands(rs, p, N):
    """B and E uniform in +-1/2, G in +-1, the temperatures TEMPS.  P's rows of 2000 and more entries make dt a sum with more cancellation
    than the 400 x 300 matrix of test_spmm_edge_softagg_gpu.py has: with B and E in +-1 its fp32 emulation on P reaches 0.47 of _close's
    limit (add_relu's dt, 8 partial states per row, the fewest a long row gets); halved, it stays below 0.12 for every op
    (tests/test_spmm_edge_softagg_tolerance.py).  The inputs are shrunk, not the limit widened."""
    half = np.float32(0.5)
    return rand(rs, p.K, N) * half, rand(rs, p.nnz, N) * half, rand(rs, p.M, N), es.temps(N)


def names_ok(p, op, fwd, bwd):
    """every pass over P runs the long-row kernel: the forward and the row pass on P, the column pass (there is none for copy) on P^T"""
    assert fwd == "spmm_edge_softagg" + ("+long_rows" if p.long_rows else ""), fwd
    assert bwd == "spmm_edge_softagg_backward" + ("+long_rows" if p.long_rows or op != "copy" else ""), bwd


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("N", WIDTHS)
def test_edge_softagg(sx, N, name):
    p = pat(name)
    a = es.EdgeSoftAbi(sx, p.rp, p.ci, np.ones(p.nnz, np.float32), p.M, p.K)
    for op in es.OPS:
        rs = rng("edge_softagg", op, N, name)
        B, E, G, t = operands(rs, p, N)
        names = [g for g in es.GRADS if not (op == "copy" and g == "dB")]
        C, lse, _, _ = a.fwd(op, B, E, t)
        fwd = a.eng.last_kernel()
        got = a.bwd(op, B, E, t, C, lse, G, want=names)
        names_ok(p, op, fwd, a.eng.last_kernel())
        wC, wL, wdB, wdE, wdt = es.reference(op, p.rp, p.ci, B, E, t, G, p.K)
        print(op, "C error / limit", es.limit_ratio(C, wC), "lse", es.limit_ratio(lse, wL))
        assert _close(C, wC), op
        assert es.lse_close(lse, wL), op
        for k, want in (("dB", wdB), ("dE", wdE), ("dt", wdt)):
            if k in names:
                print(op, k, "error / limit", es.limit_ratio(got[k], want))
                assert _close(got[k], want), (op, k)
        empty_rows_ok(p, C, lse)
    a.eng.close()


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("N", WIDTHS)
def test_uniform_scores_edge_softagg(sx, N, name):
    """t = 0: the weights are 1 / n.  mul: int_values times +-1; add: +-3 / +-4 plus +-1, an integer of magnitude 2 .. 5; copy: int_values"""
    p, rs = pat(name), rng("u-edge_softagg", N, name)
    sign = lambda *shape: rs.choice([-1, 1], shape).astype(np.float32)   # noqa: E731
    cases = {"mul": (int_values(rs, p.K, N), sign(p.nnz, N)),
             "add": ((rs.randint(3, 5, (p.K, N)) * sign(p.K, N)).astype(np.float32), sign(p.nnz, N)),
             "copy": (None, int_values(rs, p.nnz, N))}
    a = es.EdgeSoftAbi(sx, p.rp, p.ci, np.ones(p.nnz, np.float32), p.M, p.K)
    for op, (B, E) in cases.items():
        C, lse, _, _ = a.fwd(op, B, E, np.zeros(N, np.float32))
        assert a.eng.last_kernel() == "spmm_edge_softagg" + ("+long_rows" if p.long_rows else "")
        mean_is_exact(p, C, lse, es.messages32(op, B, E, p.ci))
    a.eng.close()
