"""The tolerance of the vector attention's GPU tests holds for fp32 arithmetic as such (no GPU needed): the CPU emulation of the kernels'
float32 operations in tests/test_vector_attention_gpu.py against its float64 reference, on that module's own inputs (the entries of a
row taken one after the other) and on those of tests/test_vector_attention_dealing_gpu.py (a long row dealt to 8 partial states).
Every mode must stay at or below HALF of _close's limit (rtol 2e-4) for C, lse and the gradients -- the other half is left to the
kernels' own summation orders and to the hardware's exp and log.  The ratios are quoted in the two modules' docstrings."""
import numpy as np
import pytest

import test_vector_attention_dealing_gpu as deal
import test_vector_attention_gpu as va
from test_pattern_dealing_gpu import pat, rng

NAMES = ("C", "lse", "dS", "dV", "dD")


def worst_ratio(mode, got, want):
    worst = 0.0
    for name, g, w in zip(NAMES, got, want):
        if w is None:
            assert g is None and name not in va.grads_of(mode)
            continue
        ratio = va.limit_ratio(g, w)
        print(mode, name, "error / limit %.3f" % ratio, "max |ref| %.3g" % float(np.abs(w[np.isfinite(w)]).max()))
        worst = max(worst, ratio)
    print(mode, "largest error / limit %.3f" % worst)
    return worst


@pytest.mark.parametrize("mode", list(va.MODES))
def test_fp32_emulation_is_within_half_the_limit(mode):
    N = 16
    rp, ci, v, M, K, S, V, D, G = va.inputs(N)
    want = va.reference(mode, rp, ci, S, V, D, G, K)
    got = va.emulate(mode, rp, ci, S, V, D, G, K)
    assert worst_ratio(mode, got, want) <= 0.5


@pytest.mark.parametrize("mode", list(va.MODES))
def test_fp32_emulation_on_the_dealing_pattern(mode):
    """tests/test_vector_attention_dealing_gpu.py's operands on P (rows of 2046, 2048 and 2500 entries), a long row dealt to 8 partial
    states: the fewest the kernels give one (a wavefront of 8-lane slots)"""
    N, p = 8, pat("P")
    S, V, D, G = deal.operands(rng("vector_attention", mode, N, "P"), p, N)
    want = va.reference(mode, p.rp, p.ci, S, V, D, G, p.K)
    got = va.emulate(mode, p.rp, p.ci, S, V, D, G, p.K, slots=8)
    assert worst_ratio(mode, got, want) <= 0.5
