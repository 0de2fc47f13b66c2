"""sextans_row_softmax_device / sextans_row_softmax_backward_device: softmax over the stored entries of every row of the CSR matrix on
the handle, against a float64 numpy reference computed from the same fp32 inputs (s = scale * x rounded to fp32, as specified).

Bounds (u = 2^-24, n the row length, S = max |s| over the row), derived, not measured:
  forward   |p - p64| <= 2 (min(n, 2048) + 8 S + 8) u p64 + 1e-37: one rounding of s and of s - m moves the exponent by at most 4 S u, the
            exp2-of-a-product form adds at most 2 |s - m| u <= 4 S u, a sum whose longest chain is 2048 adds of positive terms has relative
            error <= 2048 u, the exp and the division take the + 8, the factor 2 covers second-order terms;
            |sum_row p - 1| <= 2 (min(n, 2048) + 8) u
  backward  |dx - dx64| <= 2 (min(n, 2048) + 8) u |scale| p (|g| + sum_row p |g|) + 1e-37, dx64 from the fp32 p handed in."""
import os

import numpy as np
import pytest

from util import CASES, random_csr

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SCALES = [1.0, 0.125, -0.7]
INVALID, STATE = 9, 12


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def hub_matrix():
    """a single row of 300 000 entries next to short rows"""
    rs = np.random.RandomState(3)
    M, K = 2000, 300000
    lens = rs.poisson(5, M)
    lens[700] = 300000
    rp = np.zeros(M + 1, np.int32)
    rp[1:] = np.cumsum(lens)
    ci = rs.randint(0, K, rp[-1]).astype(np.int32)
    ci[rp[700]:rp[701]] = np.arange(300000, dtype=np.int32)
    return rp, ci, np.ones(rp[-1], np.float32), M, K


def matrices(sx):
    from sextans_amd import api
    rs = np.random.RandomState(1)
    rp, ci, v = random_csr(rs, 3000, 2200, 11, empty_frac=0.1, long_rows=2)
    yield "random", rp, ci, v, 3000, 2200
    rp, ci, v = api.gen_fem3d_host(14, 13, 12, 3, 7)
    yield "fem", rp, ci, v, 14 * 13 * 12 * 3, 14 * 13 * 12 * 3
    rp, ci, v = api.gen_powerlaw_host(20000, 20000, 3, 120, 15000, 11)
    yield "powerlaw", rp, ci, v, 20000, 20000
    rp, ci, v, M, K = hub_matrix()
    yield "hub", rp, ci, v, M, K
    for name in ("one_by_one", "no_entries"):
        rp, ci, v, M, K, nnz = sx.read_suitsparse_matrix(os.path.join(CASES, name + ".mtx"))
        yield name, rp, ci, v, M, K


def segments(rp):
    lens = np.diff(rp).astype(np.int64)
    starts = rp[:-1][lens > 0].astype(np.int64)
    rows = np.repeat(np.arange(len(lens)), lens)        # row of every entry
    seg = np.cumsum(lens > 0)[rows] - 1 if len(rows) else rows   # index of the entry's row among the non-empty rows
    return lens, starts, rows, seg


def forward_ref(rp, x, scale):
    """(p64, n per entry, S per entry) in float64 from s = fp32(scale * x)"""
    lens, starts, rows, seg = segments(rp)
    if len(x) == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0)
    with np.errstate(all="ignore"):
        s = (np.float32(scale) * x.astype(np.float32)).astype(np.float32).astype(np.float64)
        m = np.maximum.reduceat(s, starts)
        t = np.exp(s - m[seg])
        Z = np.add.reduceat(t, starts)
        S = np.maximum.reduceat(np.abs(s), starts)
        return t / Z[seg], lens[rows].astype(np.float64), S[seg]


def backward_ref(rp, p, g, scale):
    lens, starts, rows, seg = segments(rp)
    if len(p) == 0:
        return np.zeros(0), np.zeros(0)
    p64, g64 = p.astype(np.float64), g.astype(np.float64)
    d = np.add.reduceat(p64 * g64, starts)
    dabs = np.add.reduceat(p64 * np.abs(g64), starts)
    sc = float(np.float32(scale))
    dx = sc * p64 * (g64 - d[seg])
    bound = 2 * (np.minimum(lens[rows], 2048) + 8) * U * abs(sc) * p64 * (np.abs(g64) + dabs[seg]) + 1e-37
    return dx, bound


def dev(a):
    import torch
    t = torch.empty(max(a.size, 1) + 4, dtype=torch.float32, device="cuda")[:max(a.size, 1)]   # (16-byte aligned base, room behind the end)
    if a.size:
        t[:a.size] = torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    return t


def run_fwd(e, x, scale, inplace=False, stream=None):
    import torch
    dx = dev(x)
    dp = dx if inplace else torch.full_like(dx, -9.0)
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        e.row_softmax_device(scale, dx.data_ptr(), dp.data_ptr(), st.cuda_stream)
    torch.cuda.synchronize()
    return dp.cpu().numpy()[:x.size]


def run_bwd(e, p, g, scale, alias=None, stream=None):
    import torch
    dp, dg = dev(p), dev(g)
    dd = dg if alias == "g" else dp if alias == "p" else torch.full_like(dp, -9.0)
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        e.row_softmax_backward_device(scale, dp.data_ptr(), dg.data_ptr(), dd.data_ptr(), st.cuda_stream)
    torch.cuda.synchronize()
    return dd.cpu().numpy()[:p.size]


def test_forward_and_backward_against_float64(sx):
    for name, rp, ci, v, M, K in matrices(sx):
        rs = np.random.RandomState(len(name))
        nnz = len(ci)
        lens = np.diff(rp)
        long_rows = bool(np.any((lens > 0) & (rp[1:] - (rp[:-1] & ~3) > 2048)))   # (counted from the row's 16-byte aligned start)
        with sx.Engine(0) as e:
            e.set_matrix_csr(M, K, rp, ci, v)
            for scale in SCALES:
                x = rs.uniform(-30, 30, nnz).astype(np.float32)
                p = run_fwd(e, x, scale)
                p64, n, S = forward_ref(rp, x, scale)
                err = np.abs(p.astype(np.float64) - p64)
                bound = 2 * (np.minimum(n, 2048) + 8 * S + 8) * U * p64 + 1e-37
                worst = float((err / bound).max()) if nnz else 0.0
                print(f"{name} scale={scale}: forward worst error / bound = {worst:.3f}")
                assert np.all(err <= bound), (name, scale, worst)
                if nnz:
                    _, starts, rows, seg = segments(rp)
                    sums = np.add.reduceat(p.astype(np.float64), starts)
                    ln = lens[lens > 0]
                    assert np.all(np.abs(sums - 1.0) <= 2 * (np.minimum(ln, 2048) + 8) * U), (name, scale)
                    one = lens[rows] == 1
                    assert np.all(p[one].view(np.uint32) == np.float32(1.0).view(np.uint32)), (name, scale)
                    assert e.last_kernel() == ("row_softmax+long_rows" if long_rows else "row_softmax")
                g = rs.uniform(-1, 1, nnz).astype(np.float32)
                dx = run_bwd(e, p, g, scale)
                dx64, bb = backward_ref(rp, p, g, scale)
                errb = np.abs(dx.astype(np.float64) - dx64)
                worst = float((errb / bb).max()) if nnz else 0.0
                print(f"{name} scale={scale}: backward worst error / bound = {worst:.3f}")
                assert np.all(errb <= bb), (name, scale, worst)
                if nnz:
                    assert np.all(dx[one] == 0.0), (name, scale)     # a row of one entry: dx = +-0
                    assert e.last_kernel() == ("row_softmax_backward+long_rows" if long_rows else "row_softmax_backward")


def test_device_matrix_is_validated_and_served(sx):
    import torch
    rs = np.random.RandomState(5)
    M, K = 1500, 900
    rp, ci, v = random_csr(rs, M, K, 9)
    drp, dci, dv = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(v).cuda()
    x = rs.uniform(-30, 30, len(ci)).astype(np.float32)
    with sx.Engine(0) as e, sx.Engine(0) as e2:
        e.set_matrix_csr_device(M, K, len(ci), drp.data_ptr(), dci.data_ptr(), dv.data_ptr())
        e2.set_matrix_csr(M, K, rp, ci, v)
        assert same(run_fwd(e, x, 0.5), run_fwd(e2, x, 0.5))
        bad = rp.copy(); bad[10] = bad[11] + 3                      # row_ptr not monotone
        dbad = torch.from_numpy(bad).cuda()
        e.set_matrix_csr_device(M, K, len(ci), dbad.data_ptr(), dci.data_ptr(), dv.data_ptr())
        with pytest.raises(sx.SextansError):
            run_fwd(e, x, 0.5)


def special_matrix():
    """rows: [1, -inf, 2] | [-inf, -inf] | [+inf, 1] | [nan, 1, 2] | empty | [5] | 5000 entries, the first 2500 -inf | 3000 x -inf |
    4000 entries with one NaN | [0.5, -inf]"""
    inf = np.float32(np.inf)
    rs = np.random.RandomState(2)
    long_a = rs.uniform(-3, 3, 5000).astype(np.float32); long_a[:2500] = -inf
    long_b = np.full(3000, -inf, np.float32)
    long_c = rs.uniform(-3, 3, 4000).astype(np.float32); long_c[3100] = np.nan
    rows = [np.array([1, -inf, 2], np.float32), np.array([-inf, -inf], np.float32), np.array([inf, 1], np.float32),
            np.array([np.nan, 1, 2], np.float32), np.zeros(0, np.float32), np.array([5], np.float32), long_a, long_b, long_c,
            np.array([0.5, -inf], np.float32)]
    rp = np.zeros(len(rows) + 1, np.int32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    x = np.concatenate(rows)
    ci = np.concatenate([np.arange(len(r), dtype=np.int32) for r in rows])
    return rp, ci, x, rows


def test_special_values(sx):
    rp, ci, x, rows = special_matrix()
    zero = np.float32(0.0).view(np.uint32)
    with sx.Engine(0) as e:
        e.set_matrix_csr(len(rows), 5000, rp, ci, np.ones(len(ci), np.float32))
        p = run_fwd(e, x, 1.0)
        assert e.get_stat("softmax_long_rows") == 3
        r = [p[rp[i]:rp[i + 1]] for i in range(len(rows))]
        # -inf beside finite entries: exactly +0.0f, the rest a softmax
        assert r[0][1].view(np.uint32) == zero and abs(float(r[0][0]) + float(r[0][2]) - 1.0) < 1e-6 and r[0][2] > r[0][0] > 0
        assert r[9][1].view(np.uint32) == zero and r[9][0].view(np.uint32) == np.float32(1.0).view(np.uint32)
        # only -inf, a +inf, a NaN: NaN for the whole row
        for i in (1, 2, 3, 7, 8):
            assert np.all(np.isnan(r[i])), i
        assert r[5].view(np.uint32)[0] == np.float32(1.0).view(np.uint32)
        # long row whose first chunk holds only -inf: +0 there, finite softmax behind
        assert np.all(r[6][:2500].view(np.uint32) == zero)
        p64, n, S = forward_ref(np.array([0, 2500], np.int32), rows[6][2500:], 1.0)
        assert np.all(np.abs(r[6][2500:] - p64) <= 2 * (2048 + 8 * S + 8) * U * p64 + 1e-37)


def test_bits_do_not_depend_on_form_run_stream_or_mode(sx):
    import torch
    for name, rp, ci, v, M, K in matrices(sx):
        if name not in ("random", "hub"):
            continue
        rs = np.random.RandomState(9)
        x = rs.uniform(-30, 30, len(ci)).astype(np.float32)
        g = rs.uniform(-1, 1, len(ci)).astype(np.float32)
        with sx.Engine(0) as e, sx.Engine(0) as ef:
            e.set_matrix_csr(M, K, rp, ci, v)
            ef.set_option("mode", 1)                  # SEXTANS_MODE_FAST
            ef.set_matrix_csr(M, K, rp, ci, v)
            p = run_fwd(e, x, -0.7)
            dx = run_bwd(e, p, g, -0.7)
            assert same(run_fwd(e, x, -0.7, inplace=True), p), name
            assert same(run_bwd(e, p, g, -0.7, alias="g"), dx) and same(run_bwd(e, p, g, -0.7, alias="p"), dx), name
            assert same(run_fwd(e, x, -0.7), p) and same(run_bwd(e, p, g, -0.7), dx), name
            s2 = torch.cuda.Stream()
            assert same(run_fwd(e, x, -0.7, stream=s2), p) and same(run_bwd(e, p, g, -0.7, stream=s2), dx), name
            assert same(run_fwd(ef, x, -0.7), p) and same(run_bwd(ef, p, g, -0.7), dx), name


def test_lifecycle_prepare_capture_and_new_pattern(sx):
    import torch
    rp, ci, v, M, K = hub_matrix()
    nnz = len(ci)
    rs = np.random.RandomState(4)
    x0 = rs.uniform(-30, 30, nnz).astype(np.float32)
    x1 = rs.uniform(-30, 30, nnz).astype(np.float32)
    g = rs.uniform(-1, 1, nnz).astype(np.float32)
    with sx.Engine(0) as e:
        e.set_matrix_csr(M, K, rp, ci, v)
        assert e.get_stat("softmax_long_rows") == 0          # (nothing built yet)
        before = e.get_stat("device_bytes")
        e.prepare(16, rowmajor=True, transposed=True)
        assert e.get_stat("softmax_long_rows") == 1
        prepared = e.get_stat("device_bytes")
        assert prepared > before
        want_p = [run_fwd(e, x, 0.125) for x in (x0, x1)]
        want_d = [run_bwd(e, p, g, 0.125) for p in want_p]
        assert e.last_kernel() == "row_softmax_backward+long_rows"
        assert e.get_stat("device_bytes") == prepared
        # forward + backward captured, replayed with x rewritten: the bits of the direct calls
        dx, dg = dev(x0), dev(g)
        dp, dd = torch.empty_like(dx), torch.empty_like(dx)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            st = torch.cuda.current_stream().cuda_stream
            e.row_softmax_device(0.125, dx.data_ptr(), dp.data_ptr(), st)
            e.row_softmax_backward_device(0.125, dp.data_ptr(), dg.data_ptr(), dd.data_ptr(), st)
        for k, x in enumerate((x0, x1, x0)):
            dx[:nnz] = torch.from_numpy(x).cuda()
            graph.replay()
            torch.cuda.synchronize()
            assert same(dp.cpu().numpy()[:nnz], want_p[k % 2]) and same(dd.cpu().numpy()[:nnz], want_d[k % 2]), k
        assert e.get_stat("device_bytes") == prepared
        # a value refresh leaves the tables alone; another pattern drops them and gets its own result
        e.update_values(np.full(nnz, 2.0, np.float32))
        assert e.get_stat("softmax_long_rows") == 1 and same(run_fwd(e, x0, 0.125), want_p[0])
        rp2, ci2, v2 = random_csr(np.random.RandomState(6), 800, 500, 7)
        e.set_matrix_csr(800, 500, rp2, ci2, v2)
        assert e.get_stat("softmax_long_rows") == 0
        x2 = rs.uniform(-30, 30, len(ci2)).astype(np.float32)
        p2 = run_fwd(e, x2, 1.0)
        assert e.last_kernel() == "row_softmax" and e.get_stat("softmax_long_rows") == 0
        p64, n, S = forward_ref(rp2, x2, 1.0)
        assert np.all(np.abs(p2 - p64) <= 2 * (np.minimum(n, 2048) + 8 * S + 8) * U * p64 + 1e-37)
        with sx.Engine(0) as fresh:
            fresh.set_matrix_csr(800, 500, rp2, ci2, v2)
            assert same(run_fwd(fresh, x2, 1.0), p2)


def test_errors(sx):
    import torch
    from sextans_amd import api
    t = torch.zeros(4096, device="cuda")
    a = t.data_ptr()
    st = torch.cuda.current_stream().cuda_stream

    def code(fn, *args):
        with pytest.raises(sx.SextansError) as ei:
            fn(*args)
        return ei.value.code

    with sx.Engine(0) as e:
        assert code(e.row_softmax_device, 1.0, a, a, st) == STATE                          # before set_matrix
        assert code(e.row_softmax_backward_device, 1.0, a, a + 4096, a + 8192, st) == STATE
        bcol, bval = api.gen_bell_host(64, 64, 2, 5)
        e.set_matrix_bell(64, 64, 2, bcol, bval)
        assert code(e.row_softmax_device, 1.0, a, a, st) == STATE                          # a blocked-ELL matrix is not covered
        rp, ci, v = random_csr(np.random.RandomState(1), 100, 80, 5)
        e.set_matrix_csr(100, 80, rp, ci, v)
        assert code(e.row_softmax_device, 1.0, None, a, st) == INVALID
        assert code(e.row_softmax_device, 1.0, a, None, st) == INVALID
        assert code(e.row_softmax_device, 1.0, a + 4, a, st) == INVALID
        assert code(e.row_softmax_device, 1.0, a, a + 8, st) == INVALID
        assert code(e.row_softmax_backward_device, 1.0, a, None, a, st) == INVALID
        assert code(e.row_softmax_backward_device, 1.0, a, a + 4096, a + 8196, st) == INVALID
        e.row_softmax_device(1.0, a, a, st)                                                 # (and the handle still works)
        torch.cuda.synchronize()
        e.set_matrix_csr(3, 3, np.zeros(4, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
        e.row_softmax_device(1.0, None, None, st)                                           # nnz == 0: OK, nothing to do
        e.row_softmax_backward_device(1.0, None, None, None, st)
