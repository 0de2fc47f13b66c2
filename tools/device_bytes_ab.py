"""Stat "device_bytes" from several library builds after identical calls, each build in its own process:

    python tools/device_bytes_ab.py tools/bin/libsextans_parent.so sextans_amd/lib/libsextans_amd.so [--plan-build]

Workloads: nasa4704 at N = 16 (a column-major, a row-major and a transposed row-major SpMM, a row softmax, a value refresh: the calls of
tests/test_device_bytes_gpu.py), a randomly renumbered 3-dof FEM mesh of 65 856 rows (graph-clustered plan, column-major and row-major
calls) and a small blocked-ELL matrix.  One line per checkpoint and build, so that a difference can be read off the call that made it
(profiles/device_bytes_accounting.txt).  --plan-build: also "plan_build_s" of the 4M-row FEM matrix (api.gen_fem3d_device) at N = 16."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 16


def child(libpath, plan_build):
    sys.path.insert(0, ROOT)
    import sextans_amd.api as api
    api.LIB_PATH = os.path.join(ROOT, libpath)
    import numpy as np
    import torch
    from sextans_amd import meshgen
    tag = os.path.basename(libpath)
    st = torch.cuda.current_stream().cuda_stream
    rnd = lambda n: torch.rand(n, device="cuda") - 0.5

    def say(e, what, where):
        torch.cuda.synchronize()
        print(f"{tag:28s} {what:14s} {where:34s} {int(e.get_stat('device_bytes')):>12d}", flush=True)

    def csr_calls(e, what, M, K, nnz, transposed):
        B, C = rnd(K * N), rnd(M * N)
        e.spmm_device(N, 1.0, B.data_ptr(), K, 0.5, C.data_ptr(), C.data_ptr(), M, st); say(e, what, "column-major SpMM")
        e.spmm_device_rm(N, 1.0, B.data_ptr(), N, 0.5, C.data_ptr(), N, C.data_ptr(), N, st); say(e, what, "row-major SpMM")
        if not transposed:
            return
        Bt, Ct = rnd(M * N), rnd(K * N)
        e.spmm_t_device_rm(N, 1.0, Bt.data_ptr(), N, 0.5, Ct.data_ptr(), N, Ct.data_ptr(), N, st); say(e, what, "transposed row-major SpMM")
        x, p = rnd(nnz), torch.empty(nnz, device="cuda")
        e.row_softmax_device(0.125, x.data_ptr(), p.data_ptr(), st); say(e, what, "row softmax")
        e.update_values_device(x.data_ptr(), st); say(e, what, "update_values_device")

    rp, ci, v, M, K, nnz = api.read_suitsparse_matrix(os.path.join(ROOT, "matrices", "nasa4704", "nasa4704.mtx"))
    with api.Engine(0) as e:
        e.set_matrix_csr(M, K, rp, ci, v); say(e, "nasa4704", f"set_matrix_csr M={M} nnz={nnz}")
        csr_calls(e, "nasa4704", M, K, nnz, True)

    nx = 28
    M = nx ** 3 * 3
    rp, ci, v = api.gen_fem3d_host(nx, nx, nx, 3, 7)
    rp, ci, v = meshgen.permute_symmetric(rp, ci, v, M, meshgen.node_permutation(M // 3, 3, 1))
    with api.Engine(0) as e:
        e.set_matrix_csr(M, M, rp, ci, v); say(e, "fem28 random", f"set_matrix_csr M={M} nnz={len(ci)}")
        csr_calls(e, "fem28 random", M, M, len(ci), False)
        print(f"{tag:28s} fem28 random   row_cluster={int(e.get_stat('row_cluster'))} panel_blocks={int(e.get_stat('panel_blocks'))} "
              f"panel_blocks_clustered={int(e.get_stat('panel_blocks_clustered'))}", flush=True)

    Mb, Kb, W, Nb = 512, 768, 5, 64
    col, val = api.gen_bell_host(Mb, Kb, W, 3)
    with api.Engine(0) as e:
        e.set_matrix_bell(Mb, Kb, W, col, val); say(e, "bell 512x768x5", "set_matrix_bell")
        B = torch.zeros(Kb * Nb, dtype=torch.bfloat16, device="cuda"); Cb = torch.zeros(Mb * Nb, device="cuda")
        e.spmm_bell_device(Nb, 1.0, B.data_ptr(), Kb, 0.0, Cb.data_ptr(), Cb.data_ptr(), Mb, st); say(e, "bell 512x768x5", "spmm_bell_device N=64")

    if plan_build:
        dims = (110, 110, 110, 3)
        M = dims[0] * dims[1] * dims[2] * dims[3]
        p = api.gen_fem3d_device(0, *dims, 3)
        with api.Engine(0) as e:
            e.set_matrix_csr_device(M, M, p[3], *p[:3])
            e.prepare(N)
            torch.cuda.synchronize()
            print(f"{tag:28s} fem 4M rows    plan_build_s {e.get_stat('plan_build_s'):.4f}  device_bytes {int(e.get_stat('device_bytes'))}", flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2], "--plan-build" in sys.argv)
    else:
        libs = [a for a in sys.argv[1:] if not a.startswith("--")]
        extra = [a for a in sys.argv[1:] if a.startswith("--")]
        for lib in libs:
            rc = subprocess.run([sys.executable, __file__, "--child", lib] + extra).returncode
            if rc:
                sys.exit(rc)   # (nothing more is started on the GPU after a failure)
