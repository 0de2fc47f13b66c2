"""Blocked-ELL bf16 MFMA kernels, every variant, pinned EXACTLY with integer operands.

The argument: integers of magnitude <= 4 are exact in bf16, their products (<= 16) are exact in fp32, and every partial sum of the at most
32 * 257 products of one output element has magnitude <= 131 584 < 2^24 -- so the fp32 accumulation of the MFMA is exact in whatever
order the hardware adds.  alpha and beta are powers of two from {1, -2, 0.5, 4} (and beta = 0), C_in is integer with |c| <= 1024:
alpha * acc, beta * c and their sum (a multiple of 0.5 below 2^23) are exact as well, fused or not.  Hence C_out must EQUAL the integer
computation bit for bit on every kernel variant; a single lost, doubled or misplaced product cannot hide.  Each case asserts the
magnitude bound for its own inputs on the CPU before it trusts the equality.  The reference is a float64 BLAS product of each block
row's blocks with the block rows of B they touch (exact for these magnitudes); nothing of size K x N is built where K is large.

Every run reads B from a buffer with ldb = K + 8 whose padding holds bf16 NaN, writes C_out into a buffer with ldc = M + 3 filled with a
poison pattern that must survive, and reads C_in at ldc_in = M + 5; the packed, in-place (C_in == C_out) run must give the same bits.
The stat "bell_variant" says which kernel ran: 1 / 2 / 4 = spmm_bell_mfma<NSUB>, 8 = _n256, 9 = _shared."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POISON = 0xFFA5C3E1          # a NaN with a payload: no kernel computes it
BF16_NAN = 0x7FC0
BITMAP_RANGE = 1024 * 32     # spmm_bell_mfma_shared: a workgroup whose block columns span at most this many takes the bitmap, else the sort
MAX_UNION, MAX_ROWCOLS, SH_ROWS = 1024, 2048, 8   # kShMaxUnion, kShMaxRowCols, kShRows
SCALARS = [(1.0, -2.0), (-2.0, 0.5), (0.5, 4.0), (4.0, 1.0), (-2.0, 0.0), (0.5, -2.0), (4.0, 0.5), (1.0, 4.0)]
NAMES = {9: "spmm_bell_mfma_shared"}
DEFAULTS = dict(bell_shared=-1, bell_wide=1, bell_generation=0)


def scalars(i):
    return SCALARS[i % len(SCALARS)]


def to_bf16(x):
    f = np.ascontiguousarray(x, np.float32)
    u = f.view(np.uint32)
    assert not np.any(u & 0xFFFF)                                       # exactly representable
    return (u >> 16).astype(np.uint16)


@contextlib.contextmanager
def options(engine, **kw):
    try:
        for k, v in {**DEFAULTS, **kw}.items():
            engine.set_option(k, v)
        yield
    finally:
        for k, v in DEFAULTS.items():
            engine.set_option(k, v)


class Case:
    """Integer blocked-ELL problem on block columns bc2 (block rows x W, -1 = empty slot).  `touched`: the block rows of B that hold
    values (default: all of them; the others are zero and never materialised on the host)."""

    def __init__(self, seed, bc2, K, N, touched=None):
        rs = np.random.RandomState(seed)
        bc2 = np.ascontiguousarray(bc2, np.int32)
        self.mb, self.W = bc2.shape
        self.M, self.K, self.N, self.bc2 = self.mb * 32, K, N, bc2
        assert K % 32 == 0 and bc2.max() < K // 32 and bc2.min() >= -1
        self.touched = np.arange(K // 32) if touched is None else np.asarray(sorted(touched))
        cmap = np.full(K // 32, -1, np.int64)
        cmap[self.touched] = np.arange(len(self.touched))
        assert np.all(cmap[bc2[bc2 >= 0]] >= 0)
        # (the slots of empty entries hold values too: a kernel that multiplied one would be caught)
        self.A = rs.randint(-4, 5, (self.mb, self.W, 32, 32)).astype(np.float64)
        self.A[:, :, 0, 1] = rs.choice([-4, -3, -2, -1, 1, 2, 3, 4], (self.mb, self.W))     # never all zero in a block
        self.Bt = rs.randint(-4, 5, (len(self.touched), 32, N)).astype(np.float64)
        self.Bt[:, 1, 0] = rs.choice([-4, -3, -2, -1, 1, 2, 3, 4], len(self.touched))
        self.cin = (rs.randint(1, 1025, (self.M, N)) * rs.choice([-1, 1], (self.M, N))).astype(np.float64)
        self.acc = np.zeros((self.M, N))
        asum = np.zeros((self.M, N))
        for br in range(self.mb):
            ok = bc2[br] >= 0
            if ok.any():
                a = self.A[br, ok].transpose(1, 0, 2).reshape(32, -1)            # [m][(slot, k)]
                b = self.Bt[cmap[bc2[br, ok]]].reshape(-1, N)                    # [(slot, k)][n]
                self.acc[br * 32:(br + 1) * 32] = a @ b
                asum[br * 32:(br + 1) * 32] = np.abs(a) @ np.abs(b)
        self.acc += 0.0                                                           # (an accumulator that starts at +0 never holds -0)
        # the precondition of the exactness argument, for THESE inputs: every partial sum, in any order, stays below 2^24, and the
        # epilogue's multiple of 0.5 below 2^23
        assert asum.max() < 2 ** 24 and 4 * asum.max() + 4 * np.abs(self.cin).max() < 2 ** 23
        self._dev = {}

    def want_bits(self, alpha, beta, cin=None):
        cin = self.cin if cin is None else cin
        with np.errstate(invalid="ignore"):
            w = alpha * self.acc + beta * cin
        w32 = w.astype(np.float32)
        assert np.array_equal(w32.astype(np.float64)[np.isfinite(w)], w[np.isfinite(w)])
        return np.ascontiguousarray(w32.T).view(np.uint32)                      # [n][m]

    def set_matrix(self, engine):
        engine.set_matrix_bell(self.M, self.K, self.W, self.bc2.reshape(-1), to_bf16(self.A).reshape(-1))

    def device_B(self, ldb):
        import torch
        if ldb not in self._dev:
            dB = torch.zeros((self.N, ldb), dtype=torch.int16, device="cuda")
            if ldb > self.K:
                dB[:, self.K:] = BF16_NAN
            rows = (self.touched[:, None] * 32 + np.arange(32)).reshape(-1)
            vals = torch.from_numpy(to_bf16(self.Bt).view(np.int16).reshape(-1, self.N)).cuda()
            dB[:, torch.from_numpy(rows).cuda()] = vals.T
            self._dev[ldb] = dB
        return self._dev[ldb]

    def run(self, engine, alpha, beta, padded=True, cin=None):
        """One call; returns C_out [n][ldc] as uint32.  padded: ldb = K + 8, ldc = M + 3, ldc_in = M + 5; else everything packed and
        C_in == C_out (B stays in its padded buffer where a second copy would be large)."""
        import torch
        M, K, N = self.M, self.K, self.N
        cin = self.cin if cin is None else cin
        ldb = K + 8 if padded or K * N > (1 << 26) else K
        ldc, ldc_in = (M + 3, M + 5) if padded else (M, M)
        dB = self.device_B(ldb)
        hin = np.full((N, ldc_in), np.nan, np.float32)
        hin[:, :M] = cin.T
        dCin = torch.from_numpy(hin).cuda()
        dC = torch.from_numpy(np.full((N, ldc), POISON, np.uint32).view(np.int32)).cuda() if padded else dCin
        engine.spmm_bell_device2(N, alpha, dB.data_ptr(), ldb, beta, dCin.data_ptr(), ldc_in, dC.data_ptr(), ldc,
                                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return dC.cpu().numpy().view(np.uint32)

    def check(self, engine, alpha, beta, variant, packed_too=False):
        """Bits of all of C_out, padding included, and the kernel that ran."""
        M = self.M
        want = self.want_bits(alpha, beta)
        got = self.run(engine, alpha, beta)
        assert engine.get_stat("bell_variant") == variant
        assert engine.last_kernel() == NAMES.get(variant, "spmm_bell_mfma")
        bad = np.argwhere(got[:, :M] != want)
        assert len(bad) == 0, (len(bad), bad[:4].tolist(), got[:, :M][tuple(bad[0])], want[tuple(bad[0])])
        assert np.all(got[:, M:] == POISON)
        if packed_too:
            again = self.run(engine, alpha, beta, padded=False)
            assert engine.get_stat("bell_variant") == variant
            assert np.array_equal(again, want)


def union_lengths(bc2):
    return [len(np.unique(g[g >= 0])) for g in (bc2[i:i + SH_ROWS] for i in range(0, len(bc2), SH_ROWS))]


def column_ranges(bc2):
    out = []
    for i in range(0, len(bc2), SH_ROWS):
        g = bc2[i:i + SH_ROWS]
        out.append(int(g[g >= 0].max() - g[g >= 0].min() + 1) if (g >= 0).any() else 0)
    return out


def random_rows(rs, mb, W, lo, hi, holes=0.0):
    """Ascending distinct block columns from [lo, hi) per block row, a share of the slots emptied."""
    bc2 = np.stack([np.sort(rs.choice(np.arange(lo, hi), W, replace=False)) for _ in range(mb)]).astype(np.int32)
    bc2[rs.rand(mb, W) < holes] = -1
    return bc2


# ---- a. the per-wavefront variants ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_cases():
    """M = 7 * 32, K = 20 * 32, W = 5 with a hole in the first slot of one row, in the last slot of another, and one empty block row;
    one Case (matrix, B, C_in, integer product) per N, shared by the tests below."""
    cache = {}

    def get(N):
        if N not in cache:
            bc2 = random_rows(np.random.RandomState(11), 7, 5, 0, 20)
            bc2[1, 0] = -1; bc2[4, -1] = -1; bc2[2, :] = -1
            cache[N] = Case(100 + N, bc2, 20 * 32, N)
        return cache[N]
    return get


PER_WAVEFRONT = [(32, {}, 1), (96, {}, 1), (64, {}, 2), (128, {}, 4), (256, {}, 8), (256, dict(bell_wide=0), 4),
                 (256, dict(bell_generation=3), 8)]      # bell_generation = 3 on 7 block rows: launches of 3, 3 and 1 (br_begin = 0, 3, 6)


@pytest.mark.parametrize("i", range(len(PER_WAVEFRONT)), ids=lambda i: "N%d-%s-v%d" % (PER_WAVEFRONT[i][0], "-".join(
    f"{k}{v}" for k, v in PER_WAVEFRONT[i][1].items()) or "default", PER_WAVEFRONT[i][2]))
def test_per_wavefront_variants_exact(engine, small_cases, i):
    N, opts, variant = PER_WAVEFRONT[i]
    case = small_cases(N)
    with options(engine, bell_shared=0, **opts):
        case.set_matrix(engine)
        case.check(engine, *scalars(i), variant, packed_too=True)
        case.check(engine, *scalars(i + 4), variant)                          # (i = 0 .. 6 and i + 4 cover beta = 0 with a finite C_in)


# ---- b. the shared kernel: union lengths around the prologue depth (6) and the ring (7) --------------------------------------------
def shared_run_case(nun, sparse):
    """One workgroup of 8 block rows over one run of `nun` consecutive block columns (starting at 3: the bitmap's offset is not 0).
    sparse: wavefronts without a block at some steps (the dummy A loads) and one block row without any -- the union stays `nun`."""
    rs = np.random.RandomState(1000 + 2 * nun + sparse)
    bc2 = np.tile(np.arange(3, 3 + nun, dtype=np.int32), (8, 1))
    if sparse:
        bc2[rs.rand(8, nun) < 0.4] = -1
        bc2[5, :] = -1
        for c in range(nun):                                                   # every column keeps an owner
            if not np.any(bc2[:, c] >= 0):
                bc2[(c % 7) + (c % 7 >= 5), c] = 3 + c
        assert np.all(bc2[5] == -1) and (nun == 1 or np.any(bc2[[0, 1, 2, 3, 4, 6, 7]] == -1))
    assert union_lengths(bc2) == [nun]
    return Case(2000 + 2 * nun + sparse, bc2, (3 + nun + 2) * 32, 256)


@pytest.mark.parametrize("sparse", [0, 1], ids=["full", "dummy-loads"])
@pytest.mark.parametrize("nun", [1, 2, 5, 6, 7, 8, 13, 14, 15, 22])
def test_shared_kernel_union_lengths_exact(engine, nun, sparse):
    case = shared_run_case(nun, sparse)
    with options(engine, bell_shared=1):
        case.set_matrix(engine)
        case.check(engine, *scalars(nun + sparse), 9, packed_too=(nun in (1, 7) and not sparse))


def test_shared_kernel_empty_workgroup_exact(engine):
    """16 block rows whose second group of 8 is entirely empty (nun == 0: no main loop): its rows are (alpha * 0) + (beta * C_in)."""
    bc2 = random_rows(np.random.RandomState(5), 16, 4, 0, 12, holes=0.2)
    bc2[8:] = -1
    assert union_lengths(bc2)[1] == 0
    case = Case(31, bc2, 12 * 32, 256)
    assert not case.acc[256:].any()
    with options(engine, bell_shared=1):
        case.set_matrix(engine)
        case.check(engine, 4.0, 0.5, 9, packed_too=True)
        case.check(engine, -2.0, 0.0, 9)


@pytest.mark.parametrize("mb", [11, 9 * 8 + 1], ids=["last-workgroup-of-3-rows", "10-workgroups"])
def test_shared_kernel_partial_last_workgroup_and_grid_exact(engine, mb):
    """11 block rows: the last workgroup has 3 rows (5 wavefronts without one).  73 block rows: a grid of 10 through xcd_remap."""
    rs = np.random.RandomState(mb)
    bc2 = np.stack([np.sort(rs.choice(np.arange(br // 2, br // 2 + 14), 6, replace=False)) for br in range(mb)]).astype(np.int32)
    bc2[rs.rand(mb, 6) < 0.15] = -1
    case = Case(40 + mb, bc2, (mb // 2 + 14) * 32, 256)
    with options(engine, bell_shared=1):
        case.set_matrix(engine)
        case.check(engine, *scalars(mb), 9, packed_too=True)


# ---- c. the shared kernel: both union builders ------------------------------------------------------------------------------------
def _two_ends(hi):
    return np.tile(np.r_[0:4, hi - 3:hi + 1].astype(np.int32), (8, 1))


def _unequal_wide_rows():
    """W = 80 (n_in = 640 > 512: the sort runs on P = 1024 entries), rows of unequal length over two clusters 32 769 columns apart."""
    rs = np.random.RandomState(77)
    pool = np.r_[0:60, 32700:32769]
    bc2 = np.full((8, 80), -1, np.int32)
    for r in range(8):
        n = [80, 41, 63, 0, 80, 57, 72, 49][r]
        cols = np.sort(rs.choice(pool, n, replace=False))
        slots = np.sort(rs.choice(80, n, replace=False))                       # holes anywhere, columns ascending over the filled slots
        bc2[r, slots] = cols
    bc2[0, np.flatnonzero(bc2[0] >= 0)[0]] = 0                                 # the range is exactly 32 769
    bc2[7, np.flatnonzero(bc2[7] >= 0)[-1]] = 32768
    return bc2


BUILDERS = {"bitmap-range-32768": (lambda: _two_ends(32767), False), "sort-range-32769": (lambda: _two_ends(32768), True),
            "sort-P1024-unequal-rows": (_unequal_wide_rows, True)}


@pytest.mark.parametrize("which", list(BUILDERS))
def test_shared_kernel_union_builders_exact(sx, which):
    """The bitmap covers a range of exactly 32 768 block columns; 32 769 takes the bitonic sort -- which a matrix with K > 1 M whose
    block rows share columns reaches in production.  B (K x 256 bf16, ~540 MB) exists on the device only, zero but for the touched
    block rows; the reference gathers those."""
    from sextans_amd import api
    make, sort_branch = BUILDERS[which]
    bc2 = make()
    for row in bc2:
        assert np.all(np.diff(row[row >= 0]) > 0)
    rng, = column_ranges(bc2)
    assert (rng > BITMAP_RANGE) == sort_branch and rng in (BITMAP_RANGE, BITMAP_RANGE + 1)     # the range that selects each branch
    assert union_lengths(bc2)[0] <= MAX_UNION
    K = int(bc2.max() + 1) * 32
    touched = np.unique(np.r_[bc2[bc2 >= 0], 4, bc2.max() - 4])               # + two untouched neighbours that hold values too
    case = Case(len(which), bc2, K, 256, touched=touched)
    with api.Engine(0) as e:                                                   # (its own engine: the 540 MB workspace goes with it)
        e.set_option("bell_shared", 1)
        case.set_matrix(e)
        case.check(e, -2.0, 0.5, 9, packed_too=True)


# ---- d. the capacity limits and their fallback ------------------------------------------------------------------------------------
def _capacity(which):
    if which == "union-1024":          # 8 rows x 128 pairwise disjoint columns
        return np.arange(1024, dtype=np.int32).reshape(8, 128), 9
    if which == "union-1025":          # W = 129: rows 0..6 disjoint (903), row 7 brings 122 new columns and shares 7 with row 0
        bc2 = np.empty((8, 129), np.int32)
        bc2[:7] = np.arange(7 * 129).reshape(7, 129)
        bc2[7] = np.r_[0:7, 903:1025]
        return bc2, 8
    if which == "rowcols-2048":        # W = 256: 8 * W = 2048 slots, the rows overlap: union 956
        return (np.arange(256, dtype=np.int32)[None, :] + 100 * np.arange(8, dtype=np.int32)[:, None]), 9
    if which == "rowcols-2056":        # W = 257: one slot per row too many
        return (np.arange(257, dtype=np.int32)[None, :] + 90 * np.arange(8, dtype=np.int32)[:, None]), 8
    raise KeyError(which)


@pytest.mark.parametrize("which", ["union-1024", "union-1025", "rowcols-2048", "rowcols-2056"])
def test_shared_kernel_capacity_limits_exact(engine, which):
    """bell_shared = 1 asks for the shared kernel; it runs at union = kShMaxUnion and at 8 * W = kShMaxRowCols, and one past either
    limit the engine stays on the per-wavefront kernel (N = 256: spmm_bell_mfma_n256) -- right in all four."""
    bc2, variant = _capacity(which)
    un, = union_lengths(bc2)
    assert (un <= MAX_UNION and SH_ROWS * bc2.shape[1] <= MAX_ROWCOLS) == (variant == 9)
    assert {"union-1024": un == 1024, "union-1025": un == 1025 and SH_ROWS * 129 <= MAX_ROWCOLS, "rowcols-2048": SH_ROWS * bc2.shape[1] == 2048,
            "rowcols-2056": un <= MAX_UNION}[which]
    case = Case(len(which) + un, bc2, int(bc2.max() + 1) * 32, 256)
    with options(engine, bell_shared=1):
        case.set_matrix(engine)
        case.check(engine, *scalars(un), variant)


# ---- e. beta = 0 does not mask a NaN or an infinity in C_in: every variant ---------------------------------------------------------
NONFINITE = [(32, {}, 1), (64, {}, 2), (128, {}, 4), (256, dict(bell_shared=0), 8), (256, dict(bell_shared=1), 9)]


@pytest.mark.parametrize("i", range(len(NONFINITE)), ids=lambda i: "v%d" % NONFINITE[i][2])
def test_beta_zero_propagates_nonfinite_c_in_on_every_variant(engine, i):
    """include/sextans_amd.h: (alpha * acc) + (beta * C_in) is evaluated as written, so a NaN or an infinity in C_in gives NaN in C_out at
    beta = 0 too (cpu_spmm_CSR's contract) -- the same on every variant, also in a workgroup of the shared kernel without any block."""
    N, opts, variant = NONFINITE[i]
    bc2 = random_rows(np.random.RandomState(9), 16, 4, 0, 12, holes=0.2)
    bc2[8:] = -1
    case = Case(60 + i, bc2, 12 * 32, N)
    cin = case.cin.copy()
    spots = [(0, 0, np.nan), (37, 5, np.inf), (70, N - 1, -np.inf), (255, 17, np.nan), (256, 3, np.inf), (511, N - 2, np.nan),
             (300, 20, -np.inf)]                                               # (row, column): both lane halves, first / last tiles, empty rows
    for m, n, x in spots:
        cin[m, n] = x
    with options(engine, **{"bell_shared": 0, **opts}):
        case.set_matrix(engine)
        for alpha, beta in ((1.0, 0.0), (-2.0, 0.5)):
            want = case.want_bits(alpha, beta, cin).view(np.float32)
            got = case.run(engine, alpha, beta, cin=cin)
            assert engine.get_stat("bell_variant") == variant
            gotf = got[:, :case.M].view(np.float32)
            hit = np.zeros((N, case.M), bool)
            for m, n, _ in spots:
                hit[n, m] = True
            if beta == 0.0:
                assert np.all(np.isnan(want[hit]))                             # what the contract says
            else:
                assert np.array_equal(np.isnan(want), np.isnan(np.ascontiguousarray(cin.T)))
            assert np.array_equal(np.isnan(gotf), np.isnan(want))
            assert np.array_equal(gotf[~hit].view(np.uint32), want[~hit].view(np.uint32))      # everything else: the bits
            assert np.array_equal(gotf[hit & ~np.isnan(want)], want[hit & ~np.isnan(want)])    # (+-inf at beta = 0.5)
            assert np.all(got[:, case.M:] == POISON)
