"""The attention-dropout mask on the host (sextans_dropout_keep_host, csrc/dropout_hash.h) -- the definition the fused dropout kernels
share: known answers of the hash, agreement with an independent numpy-uint64 implementation written here, the statistics of the mask,
how seed and step combine, and the argument checks of the dropout entry points, which come before any device is touched.  No GPU."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest

OK = 0
INVALID = 9
STATE = 12

M64 = (1 << 64) - 1

# (seed, step, e, h, heads) -> u, the 32 bits that are compared with thresh
KNOWN = [((0, 0, 0, 0, 1), 0xa706dd2f),
         ((0, 0, 1, 0, 1), 0x2a98f501),
         ((1, 0, 0, 0, 1), 0x5e41ab08),
         ((0, 1, 0, 0, 1), 0x5e41ab08),
         ((0x123456789ABCDEF0, 0, 5, 2, 3), 0xb796e9b1),
         ((0xFFFFFFFFFFFFFFFF, 2, 2147483646, 7, 8), 0x95fa1ef6)]

THRESH = {0.1: 429496736, 0.5: 2147483648, 0.6: 2576980480, 0.9: 3865470464}


def np_mix(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def np_u(first, count, heads, seed, step):
    """(count, heads) uint32: the hash of every (entry, head), in numpy uint64 arithmetic"""
    with np.errstate(over="ignore"):
        key = np_mix(np.array([seed & M64], np.uint64) + np.uint64(step & M64))[0]
        e = np.arange(first, first + count, dtype=np.uint64)[:, None]
        h = np.arange(heads, dtype=np.uint64)[None, :]
        return (np_mix(key + e * np.uint64(heads) + h) >> np.uint64(32)).astype(np.uint32)


def thresh_of(p):
    return int(float(np.float32(p)) * 4294967296.0)


def p_with_thresh(lo, hi):
    """a float32 p whose thresh lies in [lo, hi] (a float32 has 24 bits: thresholds are 256 apart near the top)"""
    for t in range(lo, hi + 1):
        p = np.float32(t / 4294967296.0)
        if lo <= thresh_of(p) <= hi and p < 1.0:
            return float(p)
    raise AssertionError((lo, hi))


def test_known_answers(sx):
    from sextans_amd import api
    for (seed, step, e, h, heads), u in KNOWN:
        assert int(np_u(e, 1, heads, seed, step)[0, h]) == u
        below = p_with_thresh(u - 600, u)          # thresh <= u: kept
        above = p_with_thresh(u + 1, u + 600)      # thresh > u: dropped
        assert thresh_of(below) <= u < thresh_of(above)
        assert api.dropout_keep_host(e, 1, heads, below, seed, step)[0, h] == 1, hex(u)
        assert api.dropout_keep_host(e, 1, heads, above, seed, step)[0, h] == 0, hex(u)
    for p, t in THRESH.items():
        assert thresh_of(p) == t


@pytest.mark.parametrize("heads", [1, 3, 8])
def test_equals_numpy_uint64(sx, heads):
    from sextans_amd import api
    for p in (0.0, 0.1, 0.5, 0.6, 0.9):
        for seed, step, first in ((0, 0, 1), (2024, 3, 12345), (M64, 5, (1 << 31) - 700), (0x123456789ABCDEF0, M64, 1 << 33)):
            got = api.dropout_keep_host(first, 1000, heads, p, seed, step)
            want = (np_u(first, 1000, heads, seed, step) >= np.uint32(thresh_of(p))).astype(np.uint8)
            assert got.shape == (1000, heads) and np.array_equal(got, want), (p, seed, step, first)
            if p == 0.0:
                assert got.all()


def test_seeds_are_independent(sx):
    from sextans_amd import api
    a = api.dropout_keep_host(0, 65536, 1, 0.5, 0, 0)
    b = api.dropout_keep_host(0, 65536, 1, 0.5, 1, 0)
    agree = float((a == b).mean())
    print("agreement of seeds 0 and 1:", agree)
    assert 0.45 <= agree <= 0.55


def test_kept_share(sx):
    from sextans_amd import api
    worst = 0.0
    for seed in (0, 1, 2024, M64):
        for heads in (1, 3, 8):
            n = -(-65536 // heads)
            for p in (0.1, 0.5, 0.6, 0.9):
                keep = api.dropout_keep_host(0, n, heads, p, seed, 0).ravel()[:65536]
                q = 1.0 - thresh_of(p) / 4294967296.0
                sigma = math.sqrt(q * (1.0 - q) / keep.size)
                dev = abs(float(keep.mean()) - q) / sigma
                worst = max(worst, dev)
                assert dev <= 4.0, (seed, heads, p, dev)
    print("worst deviation of the kept share: %.2f sigma" % worst)


def test_step_adds_to_the_seed(sx):
    from sextans_amd import api
    for seed, step in ((0, 1), (77, 1000), (M64, 2), (1 << 63, 1 << 63)):
        a = api.dropout_keep_host(5, 4096, 3, 0.6, seed, step)
        b = api.dropout_keep_host(5, 4096, 3, 0.6, (seed + step) & M64, 0)
        assert np.array_equal(a, b)
    assert not np.array_equal(api.dropout_keep_host(5, 4096, 3, 0.6, 0, 0), api.dropout_keep_host(5, 4096, 3, 0.6, 0, 1))


def test_keep_host_argument_checks(sx):
    from sextans_amd import api
    L = api.lib()
    buf = (C.c_uint8 * 16)()
    assert L.sextans_dropout_keep_host(0, 4, 2, 0.5, 1, 0, buf) == OK
    assert L.sextans_dropout_keep_host(0, 0, 2, 0.5, 1, 0, None) == OK
    for args in ((-1, 4, 2, 0.5), (0, -1, 2, 0.5), (0, 4, 0, 0.5), (0, 4, 2, -0.1), (0, 4, 2, 1.0), (0, 4, 2, float("nan"))):
        assert L.sextans_dropout_keep_host(*args, 1, 0, buf) == INVALID, args
    assert L.sextans_dropout_keep_host(0, 4, 2, 0.5, 1, 0, None) == INVALID


# the plain entries' arguments of tests/test_attention_abi.py, test_gat_attention_abi.py and test_gatv2_attention_abi.py: aligned
# addresses that are never dereferenced, since every call here is refused before a device is touched
ATT_F = [2, 16, 16, 0.25, 16, 32, 32, 32, 48, 32, None, 64, 32, 80]
ATT_B = [2, 16, 16, 0.25, 16, 32, 32, 32, 48, 32, None, 64, 32, 80, 96, 32, 112, 128, 32, 144, 32, 160, 32, None]
GAT_F = [2, 16, 0.2, 16, 2, 32, 2, 48, 32, None, 64, 32, 80]
GAT_B = [2, 16, 0.2, 16, 2, 32, 2, 48, 32, None, 64, 32, 80, 96, 32, 112, 128, 2, 144, 2, 160, 32, None]
V2_F = [2, 16, 0.2, 16, 32, 32, 32, 48, None, 64, 32, 80]
V2_B = [2, 16, 0.2, 16, 32, 32, 32, 48, None, 64, 32, 80, 96, 32, 112, 128, 32, 144, 32, 160, 176, None]
ENTRIES = [("sextans_attention_dropout_device", ATT_F, 12), ("sextans_attention_dropout_backward_device", ATT_B, 12),
           ("sextans_gat_attention_dropout_device", GAT_F, 11), ("sextans_gat_attention_dropout_backward_device", GAT_B, 11),
           ("sextans_gatv2_attention_dropout_device", V2_F, 10), ("sextans_gatv2_attention_dropout_backward_device", V2_B, 10)]


@pytest.mark.parametrize("fake", [False, True])
def test_abi_errors_before_any_device(sx, fake):
    """On a zeroed handle (no matrix) a valid call answers STATE and on a NULL handle INVALID, both before a device is touched; a bad p
    or a misaligned d_step is INVALID on the zeroed handle -- so it is checked before the handle's state -- and it comes before the
    leading dimensions are looked at (a bad ldo together with a good p is still INVALID, of course)."""
    from sextans_amd import api
    L = api.lib()
    h = (C.c_char * (1 << 20))()
    hp = C.addressof(h) if fake else None
    want = STATE if fake else INVALID
    for name, args, ldo_at in ENTRIES:
        fn = getattr(L, name)
        plain = getattr(L, name.replace("_dropout", ""))
        assert plain(hp, *args, None) == want, name
        assert fn(hp, *args, None, None) == want, name                       # drop == NULL
        for p in (0.0, 0.6, 0.99):
            assert fn(hp, *args, C.byref(api.Dropout(p, 5)), None) == want, (name, p)
            assert fn(hp, *args, C.byref(api.Dropout(p, 5, 4096 + 8)), None) == want, (name, p)
        for p in (-0.1, 1.0, float("nan"), 2.0, float("inf")):
            assert fn(hp, *args, C.byref(api.Dropout(p, 5)), None) == INVALID, (name, p)
        for p in (0.0, 0.6):
            assert fn(hp, *args, C.byref(api.Dropout(p, 5, 4096 + 4)), None) == INVALID, (name, p)   # d_step: 8-byte aligned
        bad = list(args)
        bad[ldo_at] = 35
        assert fn(hp, *bad, C.byref(api.Dropout(0.6, 5)), None) == INVALID, name
    d = api.Dropout(0.6, 5)
    assert L.sextans_dropout_mask_device(hp, 2, C.byref(d), 4096, None) == want
    assert L.sextans_dropout_mask_device(hp, 2, None, 4096, None) == INVALID
    assert L.sextans_dropout_mask_device(hp, 0, C.byref(d), 4096, None) == INVALID
    assert L.sextans_dropout_mask_device(hp, 2, C.byref(api.Dropout(1.0, 5)), 4096, None) == INVALID
    assert L.sextans_dropout_mask_device(hp, 2, C.byref(d), 4100, None) == INVALID


def test_python_and_torch_surfaces(sx):
    import os
    from sextans_amd import api, torch_op
    from util import ROOT
    raw = C.CDLL(api.LIB_PATH)
    for name, _, _ in ENTRIES + [("sextans_dropout_mask_device", 0, 0), ("sextans_dropout_keep_host", 0, 0)]:
        assert name in api._OPTIONAL_SYMBOLS and hasattr(raw, name), name
    for fam in ("attention", "gat_attention", "gatv2_attention"):
        for suffix in ("device", "backward_device"):
            plain = list(inspect.signature(getattr(api.Engine, "%s_%s" % (fam, suffix))).parameters)
            drop = list(inspect.signature(getattr(api.Engine, "%s_dropout_%s" % (fam, suffix))).parameters)
            assert drop == plain[:-1] + ["drop", "stream"], fam
    for name, lead in (("sparse_attention_dropout", ["A", "Q", "K", "V"]), ("gat_attention_dropout", ["A", "a_dst", "a_src", "V"]),
                       ("gatv2_attention_dropout", ["A", "x_dst", "x_src", "att"])):
        sig = inspect.signature(getattr(torch_op, name)).parameters
        assert list(sig)[:7] == lead + ["dropout", "seed", "step"], name
        assert sig["seed"].default is None and sig["step"].default is None
        assert name in torch_op.__doc__
    assert list(inspect.signature(torch_op.dropout_mask).parameters) == ["A", "heads", "p", "seed", "step"]
    for bad in (-0.1, 1.0, float("nan"), 1.5):
        with pytest.raises(ValueError):
            torch_op._check_dropout(bad)
    with open(os.path.join(ROOT, "include", "sextans_amd.h")) as f:
        text = " ".join(f.read().split())
    assert "typedef struct { float p; uint64_t seed; const uint64_t *d_step; } sextans_dropout;" in text
    assert "int sextans_dropout_mask_device(sextans_handle_t h, int heads, const sextans_dropout *drop, float *d_mult, void *stream);" in text
    assert ("int sextans_dropout_keep_host(int64_t first, int64_t count, int heads, float p, uint64_t seed, uint64_t step, uint8_t *keep);"
            in text)
    assert "float *d_lse, const sextans_dropout *drop, void *stream);" in text
