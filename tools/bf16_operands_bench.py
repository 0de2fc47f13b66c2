"""bf16 dense operands against the fp32 row-major entry point, on one GPU, seeded device generators only:

    tools/build_commit.sh HEAD~1 parent          # (before the GPU visit) the baseline a user has today -> tools/bin/libsextans_parent.so
    python tools/bf16_operands_bench.py [--out profiles/bf16_operands.jsonl] [--matrices config4,powerlaw_fast,fem] [--n 16,32,64,128]

One record per (matrix, N, variant): device-event time per call (warmed up, >= 0.5 s of timed calls over >= 5 rounds with the variants
alternated inside one process; min / median / max of the rounds), the algorithmic bytes of the variant on the route it took and the
fraction of the 8 TB/s HBM roofline they amount to (bytes / time / peak, as bench.py computes its own).
  a  fp32 spmm_device_rm of the PARENT commit's library (loaded beside this tree's)
  b  what torch_op did before: a padded fp32 copy of the bf16 B (torch_op._rowmajor) + a
  c  spmm_device_rm_bf16, C fp32
  d  spmm_device_rm_bf16, C bf16
Matrices: bench.py's default (config 4: 4 M x 4 M, 40 per row, no reuse), the 1 M-row power-law matrix in fast mode and the 4 M-row FEM
matrix of bench.py --full (the FEM matrix converts: the cost of not being native).  Every matrix runs in a child process under its
own time limit; the first failure stops the run.  A last record states the two conditions of the change: c and d are not slower than b
beyond the spread between rounds, and on config 4 at N = 32 c is faster than a by more than that spread."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK_GBS = 8000.0
PARENT_LIB = os.path.join(ROOT, "tools", "bin", "libsextans_parent.so")
ROUNDS, MIN_SECONDS = 5, 0.5


def child(matrix, Ns, out):
    sys.path.insert(0, ROOT)
    import torch
    from sextans_amd import api, torch_op
    fast = matrix == "powerlaw_fast"
    if matrix == "config4":
        M = K = 4_000_000
        p, i, v, nnz = api.gen_csr_device(0, M, K, 40.0, 4)
    elif fast:
        M = K = 1_000_000
        p, i, v, nnz = api.gen_powerlaw_device(0, M, K, 6, 120, 400_000, 7)
    else:
        M = K = 110 ** 3 * 3
        p, i, v, nnz = api.gen_fem3d_device(0, 110, 110, 110, 3, 3)
    st = torch.cuda.current_stream().cuda_stream
    e = api.Engine(0)
    P = api._bind(C.CDLL(PARENT_LIB))   # (the parent's library beside this tree's, with the same prototypes)
    ph = C.c_void_p()
    assert P.sextans_create(C.byref(ph), 0) == 0
    if fast:
        e.set_option("mode", 1)
        assert P.sextans_set_option(ph, b"mode", 1) == 0
    e.set_matrix_csr_device(M, K, nnz, p, i, v)
    assert P.sextans_set_matrix_csr_device(ph, M, K, nnz, p, i, v) == 0
    alpha, beta = 0.85, -2.06
    for N in Ns:
        B16 = torch.empty((K, N), dtype=torch.bfloat16, device="cuda")
        api.gen_uniform_bf16_device(0, B16.data_ptr(), K * N, 41, st)
        B32 = B16.float()
        C32 = torch.empty((M, N), device="cuda"); api.gen_uniform_device(0, C32.data_ptr(), M * N, 42, st)
        C16 = C32.to(torch.bfloat16)
        O32 = torch.empty((M, N), device="cuda"); O16 = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")

        def parent_rm(Bt):
            rc = P.sextans_spmm_device_rm(ph, N, alpha, Bt.data_ptr(), N, beta, C32.data_ptr(), N, O32.data_ptr(), N, st)
            assert rc == 0, rc

        variants = {
            "a": lambda: parent_rm(B32),
            "b": lambda: parent_rm(torch_op._rowmajor(B16, K, N, N)),
            "c": lambda: e.spmm_device_rm_bf16(N, alpha, B16.data_ptr(), N, beta, C32.data_ptr(), N, O32.data_ptr(), N, api.DTYPE_F32, st),
            "d": lambda: e.spmm_device_rm_bf16(N, alpha, B16.data_ptr(), N, beta, C16.data_ptr(), N, O16.data_ptr(), N, api.DTYPE_BF16, st),
        }
        e.prepare_rm_bf16(N, api.DTYPE_BF16)
        info, calls = {}, {}
        for name, f in variants.items():      # warm up (plans, workspaces), note the route, size the rounds
            n0 = e.get_stat("bf16_native_calls")
            for _ in range(3):
                f()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(); f(); f(); t1.record(); torch.cuda.synchronize()
            per = max(t0.elapsed_time(t1) / 2e3, 1e-6)
            calls[name] = max(3, int(MIN_SECONDS / ROUNDS / per) + 1)
            native = name in "cd" and e.get_stat("bf16_native_calls") > n0
            kernel = e.last_kernel() if name in "cd" else P.sextans_last_kernel(ph).decode()
            info[name] = (native, kernel)
        times = {name: [] for name in variants}
        for _ in range(ROUNDS):
            for name, f in variants.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(calls[name]):
                    f()
                t1.record(); torch.cuda.synchronize()
                times[name].append(t0.elapsed_time(t1) * 1e3 / calls[name])      # us per call
        a_bytes = 8 * nnz + 4 * (M + 1)
        copy_b = 2 * K * N + 4 * K * N                                            # bf16 B read, fp32 copy written
        by = {"a": a_bytes + 4 * K * N + 8 * M * N, "b": a_bytes + copy_b + 4 * K * N + 8 * M * N}
        by["c"] = a_bytes + 2 * K * N + 8 * M * N if info["c"][0] else by["b"]
        by["d"] = a_bytes + 2 * K * N + 4 * M * N if info["d"][0] else by["b"] + 2 * (2 * M * N + 4 * M * N)
        for name in variants:
            t = sorted(times[name])
            med = statistics.median(t)
            rec = {"matrix": matrix, "M": M, "K": K, "nnz": nnz, "N": N, "variant": name, "native": info[name][0], "kernel": info[name][1],
                   "calls_per_round": calls[name], "rounds": ROUNDS, "us_min": round(t[0], 2), "us_median": round(med, 2), "us_max": round(t[-1], 2),
                   "alg_bytes": by[name], "roofline_frac": round(by[name] / (med * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)}
            with open(out, "a") as f:
                f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec), flush=True)
        del B16, B32, C32, C16, O32, O16
        torch.cuda.empty_cache()
    e.close()
    P.sextans_destroy(ph)


def conditions(out):
    recs = {}
    with open(out) as f:
        for line in f:
            r = json.loads(line)
            if "variant" in r:
                recs[(r["matrix"], r["N"], r["variant"])] = r
    spread = lambda r: r["us_max"] - r["us_min"]
    slower = []
    for (m, n, var), r in sorted(recs.items()):
        if var in "cd" and (m, n, "b") in recs:
            b = recs[(m, n, "b")]
            if r["us_median"] > b["us_median"] + max(spread(r), spread(b)):
                slower.append([m, n, var, r["us_median"], b["us_median"]])
    res = {"record": "conditions", "c_d_not_slower_than_b": not slower, "slower": slower}
    a, c = recs.get(("config4", 32, "a")), recs.get(("config4", 32, "c"))
    if a and c:
        res["config4_N32_c_vs_a"] = {"a_us": a["us_median"], "c_us": c["us_median"], "spread_us": round(max(spread(a), spread(c)), 2),
                                     "c_faster_beyond_spread": c["us_median"] < a["us_median"] - max(spread(a), spread(c))}
    with open(out, "a") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_operands.jsonl"))
    ap.add_argument("--matrices", default="config4,powerlaw_fast,fem")
    ap.add_argument("--n", default="16,32,64,128")
    ap.add_argument("--timeout", type=int, default=420, help="seconds per matrix")
    ap.add_argument("--child", default="")
    args = ap.parse_args()
    Ns = [int(x) for x in args.n.split(",")]
    if args.child:
        return child(args.child, Ns, args.out)
    if not os.path.exists(PARENT_LIB):
        sys.exit("missing " + PARENT_LIB + ": run tools/build_commit.sh <parent commit> parent first")
    open(args.out, "w").close()
    for m in args.matrices.split(","):
        rc = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", m, "--n", args.n,
                             "--out", args.out]).returncode
        if rc != 0:
            sys.exit(f"{m}: exit status {rc} -- stopping")
    conditions(args.out)


if __name__ == "__main__":
    main()
