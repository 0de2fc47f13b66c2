"""The edge-feature multi-aggregation (sextans_spmm_edge_multi_device_rm / _backward_device_rm) on every row-dealing path of
pattern_pass.h: the 92-row pattern P of test_pattern_dealing_gpu.py (one slot group per row, several slots per row, an idle slot group,
the second walk, the long-row kernel, empty rows) and its transpose P^T, whose column pass walks P with P's own tables -- the long-row
kernel on A and on A^T, asserted through last_kernel.  Every slot width of the family: N = 8, 16, 32, 64.
  Integer operands in [-4, 4], as test_spmm_edge there: every message (|m| <= 16), square, t = Gsum + 2 m Gsq + Gmax + Gmin (|t| <= 140),
product and partial sum is an integer below 2^24 (at most 2600 terms per sum), so every summation order is exact: the sums, dB and dE
EQUAL the int64 computation; the extrema and args equal numpy's (the first of equal messages wins)."""
import numpy as np
import pytest

import test_spmm_edge_gpu as sedge
import test_spmm_edge_multi_gpu as em
from test_pattern_dealing_gpu import pat, rng

pytestmark = pytest.mark.gpu


def int_backward(op, p, B, E, args, G):
    """dB (None for copy) and dE in int64"""
    rows = np.repeat(np.arange(p.M), p.lens)
    e = np.arange(p.nnz)[:, None]
    Bc, Ei = B.astype(np.int64)[p.ci], E.astype(np.int64)
    m = Bc * Ei if op == "mul" else Bc + Ei if op == "add" else np.maximum(Bc + Ei, 0) if op == "add_relu" else Ei
    g = {k: x.astype(np.int64)[rows] for k, x in G.items()}
    t = g["sum"] + 2 * m * g["sumsq"] + np.where(args["max"][rows] == e, g["max"], 0) + np.where(args["min"][rows] == e, g["min"], 0)
    assert np.abs(t).max() <= 140
    if op == "mul":
        fB, fE = Ei, Bc
    elif op == "add_relu":
        fB = fE = (Bc + Ei > 0).astype(np.int64)
    else:
        fB = fE = np.ones_like(Ei)
    return (sedge.scatter(p.ci, fB * t, p.K) if op != "copy" else None), fE * t


@pytest.mark.parametrize("name", ["P", "PT"])
@pytest.mark.parametrize("N", [8, 16, 32, 64])
@pytest.mark.parametrize("op", list(sedge.OPS))
def test_edge_multi(sx, op, N, name):
    p, rs = pat(name), rng("edge_multi", op, N, name)
    B, E = sedge.ints(rs, p.K, N), sedge.ints(rs, p.nnz, N)
    G = {k: sedge.ints(rs, p.M, N) for k in em.VALUES}
    a = em.Abi(sx, p.rp, p.ci, np.ones(p.nnz, np.float32), p.M, p.K)
    got, _ = a.edge_forward(op, B, E)
    fwd = a.eng.last_kernel()
    m, want = em.reference(op, p.rp, p.ci, B, E)
    args = {"max": want["argmax"], "min": want["argmin"]}
    dB, dE = a.edge_backward(op, B, E, args, G)
    bwd = a.eng.last_kernel()
    a.eng.close()
    # every pass over P runs the long-row kernel: the forward and the row pass on P, the column pass (there is none for copy) on P^T
    assert fwd == "spmm_edge_multi" + ("+long_rows" if p.long_rows else ""), fwd
    assert bwd == "spmm_edge_multi_backward" + ("+long_rows" if p.long_rows or op != "copy" else ""), bwd
    for k in ("max", "min"):
        assert em.raw_equal(got[k], want[k]) and np.array_equal(got["arg" + k], want["arg" + k]), k
    m64 = m.astype(np.int64)
    rows = np.repeat(np.arange(p.M), p.lens)
    assert np.array_equal(got["sum"], sedge.scatter(rows, m64, p.M).astype(np.float32))
    assert np.array_equal(got["sumsq"], sedge.scatter(rows, m64 * m64, p.M).astype(np.float32))
    for k in em.VALUES:
        assert np.all(got[k][p.empty].view(np.uint32) == 0), k
    assert np.all(got["argmax"][p.empty] == -1) and np.all(got["argmin"][p.empty] == -1)
    wdB, wdE = int_backward(op, p, B, E, args, G)
    assert np.array_equal(dE, wdE.astype(np.float32))
    if op == "copy":
        assert dB is None
    else:
        assert np.abs(wdB).max() < 2 ** 24 and np.array_equal(dB, wdB.astype(np.float32))
