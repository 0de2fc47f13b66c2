"""Pins the oracle to the REFERENCE itself: oracle/sextans_oracle.c against the reference's own
read_suitsparse_matrix / CSC_2_CSR / cpu_spmm_CSR (oracle/_ref/libsextans_ref.so, built by
oracle/Makefile from the reference's sparse_helper.h + mmio.h).  What the reference returned for each
input is recorded in tests/golden/reference_digests.json (util.reference_digest), so these tests also
run where the reference is absent; where oracle/_ref is built, the library is checked against the recording."""
import glob
import os

import numpy as np
import pytest

from oracle.bindings import Ref
from util import ALPHA, BETA, CASES, NASA, digest, formula_B, formula_C, random_csr, reference_digest

FILES = sorted(glob.glob(os.path.join(CASES, "*.mtx"))) + [NASA]


def _csr_csc_digests(R):
    return {"dims": [R["M"], R["K"], R["nnz"]],
            "csc": digest(R["csc"][0].astype(np.int32), R["csc"][1].astype(np.int32), R["csc"][2]),
            "csr": digest(R["csr"][0].astype(np.int32), R["csr"][1].astype(np.int32), R["csr"][2])}


def _ref_load(path, capfd):
    R = Ref().load(path)
    capfd.readouterr()   # the reference prints progress lines
    return _csr_csc_digests(R)


def _ref_spmm(M, N, K, alpha, rp, ci, v, B, beta, C0):
    c = C0.copy()
    Ref().spmm(M, N, K, alpha, rp, ci, v, B, beta, c)
    return digest(c.view(np.uint32))


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(p) for p in FILES])
def test_loader_bit_identical(oracle, path, capfd):
    R = reference_digest("loader", os.path.basename(path), lambda: _ref_load(path, capfd))
    err, M, K, nnz, cp, ri, cv = oracle.read_mtx(path, 1)
    assert err == 0 and [M, K, nnz] == R["dims"]
    assert digest(cp.astype(np.int32), ri.astype(np.int32), cv) == R["csc"]
    rp, ci, v = oracle.csc_to_csr(M, K, cp, ri, cv)
    assert digest(rp.astype(np.int32), ci.astype(np.int32), v) == R["csr"]


@pytest.mark.parametrize("N", [8, 16, 40])
@pytest.mark.parametrize("seed", [0, 1])
def test_spmm_bit_identical_random(oracle, N, seed):
    rs = np.random.RandomState(100 + seed)
    M, K = 257 + 31 * seed, 300 + 17 * seed
    rp, ci, v = random_csr(rs, M, K, 9, long_rows=1)
    B = rs.uniform(-1, 1, K * N).astype(np.float32)
    C0 = rs.uniform(-1, 1, M * N).astype(np.float32)
    alpha, beta = np.float32(rs.uniform(-2, 2)), np.float32(rs.uniform(-2, 2))
    want = reference_digest("spmm_random", f"N{N}_seed{seed}", lambda: _ref_spmm(M, N, K, alpha, rp, ci, v, B, beta, C0))
    c1 = C0.copy()
    oracle.spmm(M, N, K, alpha, rp, ci, v, B, beta, c1)
    assert digest(c1.view(np.uint32)) == want


def test_spmm_bit_identical_nasa(oracle, capfd):
    M, K, nnz, rp, ci, v = oracle.load_csr(NASA)   # the reference's sequence, giving the reference's own CSR:
    assert digest(rp, ci, v) == reference_digest("loader", os.path.basename(NASA), lambda: _ref_load(NASA, capfd))["csr"]
    for N in (16, 128):
        for name, (B, C0) in (("init", (oracle.init_B(K, N), oracle.init_C(M, N))), ("formula", (formula_B(K, N), formula_C(M, N)))):
            want = reference_digest("spmm_nasa", f"N{N}_{name}", lambda: _ref_spmm(M, N, K, ALPHA, rp, ci, v, B, BETA, C0))
            c1 = C0.copy()
            oracle.spmm(M, N, K, ALPHA, rp, ci, v, B, BETA, c1)
            assert digest(c1.view(np.uint32)) == want


def test_rows_variant_equals_full(oracle):
    rs = np.random.RandomState(7)
    M, K, N = 100, 80, 16
    rp, ci, v = random_csr(rs, M, K, 6)
    B = rs.uniform(-1, 1, K * N).astype(np.float32)
    C0 = rs.uniform(-1, 1, M * N).astype(np.float32)
    full = C0.copy()
    oracle.spmm(M, N, K, ALPHA, rp, ci, v, B, BETA, full)
    part = C0.copy()
    oracle.spmm_rows(0, 37, M, N, K, ALPHA, rp, ci, v, B, BETA, part)
    oracle.spmm_rows(37, M, M, N, K, ALPHA, rp, ci, v, B, BETA, part)
    assert np.array_equal(full.view(np.uint32), part.view(np.uint32))
