"""One training step of the torch op on one GPU, piece by piece: the forward call, the transposed call (dB), the SDDMM kernel (dA), the
row-group gather kernel ("kernel" = 1) on the same operands and a full torch forward + backward step; plus the cost of the transposed
form (stat "transpose_build_s", "device_bytes" before / after).  One JSON record per run.

    python tools/train_step.py --matrix fem --N 16 --out profiles/train_step_fem_N16.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/train_step.py ...   (kernel times: tools/merge_kernel_stats.py)
    rocprofv3 --pmc COUNTERS --output-format csv -d DIR -- python tools/train_step.py --kernels-only ...   (tools/pmc_summary.py)

Matrices: "fem" = gen_fem3d_device(110, 110, 110, 3) (3.99 M rows, bench.py's rowmajor_fem_4M_N16), "config4" = gen_csr_device(4 M, 4 M,
Poisson(40), uniformly random columns; BASELINE config 4).  Times: mean of --steps calls between HIP events after --warmup calls."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", choices=["fem", "config4"], default="fem")
    ap.add_argument("--N", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true", help="the SDDMM and row-group gather kernels alone (counter passes)")
    args = ap.parse_args()
    import torch
    from sextans_amd import api, torch_op
    dev = torch.device("cuda", 0)
    N = args.N
    if args.matrix == "fem":
        p, i, v, nnz = api.gen_fem3d_device(0, 110, 110, 110, 3, 3)
        M = K = 110 ** 3 * 3
    else:
        M = K = 4_000_000
        p, i, v, nnz = api.gen_csr_device(0, M, K, 40.0, 4)
    crow = torch.empty(M + 1, dtype=torch.int32, device=dev); col = torch.empty(nnz, dtype=torch.int32, device=dev)
    val = torch.empty(nnz, dtype=torch.float32, device=dev)
    for dst, src, n in ((crow, p, (M + 1) * 4), (col, i, nnz * 4), (val, v, nnz * 4)):
        api.device_copy(0, dst.data_ptr(), src, n)
        api.device_free(0, src)
    g = torch.Generator(device=dev).manual_seed(1)
    B = torch.rand((K, N), device=dev, generator=g) * 2 - 1
    G = torch.rand((M, N), device=dev, generator=g) * 2 - 1
    C = torch.zeros((M, N), device=dev); Ct = torch.zeros((K, N), device=dev); vals = torch.empty(nnz, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.steps   # us per call

    rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": int(nnz), "N": N, "steps": args.steps}
    eng = api.Engine(0)
    eng.set_matrix_csr_device(M, K, nnz, crow.data_ptr(), col.data_ptr(), val.data_ptr())
    if args.kernels_only:
        rec["sddmm_us"] = timed(lambda: eng.sddmm_device_rm(N, 1.0, G.data_ptr(), N, B.data_ptr(), N, 0.0, None, vals.data_ptr(), stream))
        eng.close()
        gat = api.Engine(0)
        gat.set_option("kernel", 1)
        gat.set_matrix_csr_device(M, K, nnz, crow.data_ptr(), col.data_ptr(), val.data_ptr())
        rec["rowgroup_us"] = timed(lambda: gat.spmm_device_rm(N, 1.0, B.data_ptr(), N, 0.0, C.data_ptr(), N, C.data_ptr(), N, stream))
        gat.close()
        print(json.dumps(rec))
        return
    rec["forward_us"] = timed(lambda: eng.spmm_device_rm(N, 1.0, B.data_ptr(), N, 0.0, C.data_ptr(), N, C.data_ptr(), N, stream))
    rec["forward_kernel"] = eng.last_kernel()
    rec["device_bytes_before"] = eng.get_stat("device_bytes")
    t0 = time.perf_counter()
    eng.prepare(N, rowmajor=True, transposed=True, stream=stream)
    rec["transposed_prepare_wall_s"] = time.perf_counter() - t0
    rec["transpose_build_s"] = eng.get_stat("transpose_build_s")
    rec["device_bytes_after"] = eng.get_stat("device_bytes")
    rec["transposed_us"] = timed(lambda: eng.spmm_t_device_rm(N, 1.0, G.data_ptr(), N, 0.0, Ct.data_ptr(), N, Ct.data_ptr(), N, stream))
    rec["transposed_kernel"] = eng.last_kernel()
    rec["sddmm_us"] = timed(lambda: eng.sddmm_device_rm(N, 1.0, G.data_ptr(), N, B.data_ptr(), N, 0.0, None, vals.data_ptr(), stream))
    rec["sddmm_kernel"] = eng.last_kernel()
    algo = nnz * 8 + M * N * 4 + K * N * 4 + (M + 1) * 4
    rec["sddmm_algorithmic_bytes"] = algo
    rec["sddmm_fraction_of_8TBps"] = algo / (rec["sddmm_us"] * 1e-6) / 8e12
    eng.close()
    gat = api.Engine(0)
    gat.set_option("kernel", 1)
    gat.set_matrix_csr_device(M, K, nnz, crow.data_ptr(), col.data_ptr(), val.data_ptr())
    rec["rowgroup_us"] = timed(lambda: gat.spmm_device_rm(N, 1.0, B.data_ptr(), N, 0.0, C.data_ptr(), N, C.data_ptr(), N, stream))
    rec["rowgroup_kernel"] = gat.last_kernel()
    gat.close()
    A = torch.sparse_csr_tensor(crow, col, val, size=(M, K)).requires_grad_()
    Bg = B.clone().requires_grad_()

    def step():
        A.grad = None
        Bg.grad = None
        torch_op.spmm(A, Bg).backward(G)

    def fwd():
        with torch.no_grad():
            torch_op.spmm(A, Bg)

    rec["torch_forward_us"] = timed(fwd)
    rec["torch_step_us"] = timed(step)
    rec["step_over_forward"] = rec["torch_step_us"] / rec["forward_us"]
    rec["transposed_over_forward"] = rec["transposed_us"] / rec["forward_us"]
    rec["sddmm_over_rowgroup"] = rec["sddmm_us"] / rec["rowgroup_us"]
    torch_op.clear_cache()
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
