"""The tolerance of the edge-feature softmax aggregation's GPU tests holds for fp32 arithmetic as such (no GPU needed): the CPU emulation
of the kernels' float32 operations in tests/test_spmm_edge_softagg_gpu.py against its float64 reference, on that module's own inputs
(the entries of a row taken one after the other) and on those of tests/test_edge_softagg_dealing_gpu.py, at the temperatures TEMPS.
Every op must stay below HALF of _close's limit (rtol 2e-4) for C, lse and the three gradients -- the other half is left to the kernels'
own summation orders and to the hardware's exp and log.  The ratios are quoted in the two modules' docstrings."""
import numpy as np
import pytest

import test_edge_softagg_dealing_gpu as deal
import test_spmm_edge_softagg_gpu as es
from test_pattern_dealing_gpu import pat, rng


@pytest.mark.parametrize("op", list(es.OPS))
def test_fp32_emulation_is_within_half_the_limit(op):
    N = 16
    rp, ci, v, M, K, B, E, G = es.inputs(N)
    t = es.temps(N)
    assert sorted(set(t.tolist())) == sorted(set(float(x) for x in es.TEMPS))
    want = es.reference(op, rp, ci, B, E, t, G, K)
    got = es.emulate(op, rp, ci, B, E, t, G, K)
    worst = 0.0
    for name, g, w in zip(("C", "lse", "dB", "dE", "dt"), got, want):
        if w is None:
            assert g is None and op == "copy" and name == "dB"
            continue
        ratio = es.limit_ratio(g, w)
        print(op, name, "error / limit %.3f" % ratio, "max |ref| %.3g" % float(np.abs(w[np.isfinite(w)]).max()))
        worst = max(worst, ratio)
    print(op, "largest error / limit %.3f" % worst)
    assert worst <= 0.5, worst


@pytest.mark.parametrize("op", list(es.OPS))
def test_fp32_emulation_on_the_dealing_pattern(op):
    """tests/test_edge_softagg_dealing_gpu.py's operands on P (rows of 2046, 2048 and 2500 entries), a long row dealt to 8 partial states:
    the fewest the kernels give one (a wavefront of 8-lane slots)"""
    N, p = 8, pat("P")
    B, E, G, t = deal.operands(rng("edge_softagg", op, N, "P"), p, N)
    want = es.reference(op, p.rp, p.ci, B, E, t, G, p.K)
    got = es.emulate(op, p.rp, p.ci, B, E, t, G, p.K, slots=8)
    worst = max(es.limit_ratio(g, w) for g, w in zip(got, want) if w is not None)
    print(op, "largest error / limit %.3f" % worst)
    assert worst <= 0.5, worst
