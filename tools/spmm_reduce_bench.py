"""spmm_reduce(A, B, "amax") against the composition torch allows on a GPU -- materialise the (nnz, N) products val[:, None] * B[col],
then scatter_reduce(..., "amax", include_self=False) over the row index (or torch.segment_reduce over the row lengths), autograd
through it -- on the same commit, the same process and the same tensors, on one GPU.

    python tools/spmm_reduce_bench.py --matrix config4 --out profiles/spmm_reduce.jsonl     (appends one record per N)
    python tools/spmm_reduce_bench.py --matrix small --dims 16,64

Matrices: "config4" = gen_csr_device(4 M, 4 M, Poisson(40)), "fem" = gen_fem3d_device(110, 110, 110, 3) (3.99 M rows, 318 M non-zeros),
"powerlaw" = gen_powerlaw_device(1 M, 1 M, 6, 1.2, 400 000), "small" = a 200 k-row config-4 for trying the tool out.
The composition's nnz-long row-index vector (and the row lengths) are built once, outside every timed region.  Per N: the forward alone
(no autograd graph) and forward + backward (the gradient of B; --grad-a: of A's values too), each side timed between HIP events over
--rounds rounds of `reps` calls, the two sides in ALTERNATING rounds after one untimed warm-up step per side (engine, A^T and tables are
built there); reps is chosen per record so that a round lasts about --round-ms.  "ratio" = composition median / fused median (> 1: the
fused path is faster), "spread" = (max - min) / median of a side's rounds, "verdict": "fused" / "composition" when that side's slowest
round beats the other's fastest -- a difference larger than the spread between repeats -- else "undecided".
"peak_bytes": torch.cuda.max_memory_allocated over one forward + backward step of a side, above what was allocated before it.
A composition case that cannot be allocated is recorded as such ("composition": "out of memory") and the fused side is timed alone.
"spmm_sum": torch_op.spmm (the strict sum product) on the same matrix and N, for information: it does the same gathers.
"torch_sparse_mm_gpu": what torch.sparse.mm(A, B, "amax") of the installed GPU build does on a 1000-row corner of the matrix.
--fused-only times spmm_reduce alone (kernel tuning between two builds): no composition, no verdict; --tag NAME is written into every
record and says which build it timed."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", choices=["config4", "fem", "powerlaw", "small"], default="small")
    ap.add_argument("--dims", default="16,64")
    ap.add_argument("--reduce", choices=["amax", "amin"], default="amax")
    ap.add_argument("--composition", choices=["scatter", "segment"], default="scatter", help="scatter_reduce over the row index, or segment_reduce")
    ap.add_argument("--grad-a", action="store_true", help="forward + backward also takes the gradient of A's values")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-ms", type=float, default=200.0)
    ap.add_argument("--max-reps", type=int, default=8)
    ap.add_argument("--fused-only", action="store_true", help="time spmm_reduce alone (kernel tuning): no composition, no verdict")
    ap.add_argument("--tag", default="", help="written into every record as \"tag\" (names the build that was timed)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from sextans_amd import api, torch_op
    dev = torch.device("cuda", 0)
    if args.matrix == "fem":
        M = K = 110 ** 3 * 3
        p, i, v, nnz = api.gen_fem3d_device(0, 110, 110, 110, 3, 3)
    elif args.matrix == "powerlaw":
        M = K = 1_000_000
        p, i, v, nnz = api.gen_powerlaw_device(0, M, K, 6, 120, 400_000, 7)
    else:
        M = K = 4_000_000 if args.matrix == "config4" else 200_000
        p, i, v, nnz = api.gen_csr_device(0, M, K, 40.0, 4)
    crow = torch.empty(M + 1, dtype=torch.int32, device=dev); col = torch.empty(nnz, dtype=torch.int32, device=dev)
    val = torch.empty(nnz, dtype=torch.float32, device=dev)
    for dst, src, n in ((crow, p, (M + 1) * 4), (col, i, nnz * 4), (val, v, nnz * 4)):
        api.device_copy(0, dst.data_ptr(), src, n)
        api.device_free(0, src)
    A = torch.sparse_csr_tensor(crow, col, val, size=(M, K))
    vleaf = val.detach().clone()               # the composition's values: a dense leaf
    if args.grad_a:
        A.requires_grad_(); vleaf.requires_grad_()
    gen = torch.Generator(device=dev).manual_seed(1)
    lens = (crow[1:] - crow[:-1]).long()
    row = torch.repeat_interleave(torch.arange(M, device=dev), lens, output_size=int(nnz))   # built once, untimed
    col64 = col.long()
    red = args.reduce

    try:   # what the installed torch does with the sparse op itself on this device
        rows = min(M, 1000)
        n0 = int(crow[rows].item())
        A0 = torch.sparse_csr_tensor(crow[:rows + 1].clone(), col[:n0].clone(), val[:n0].clone(), size=(rows, K))
        torch.sparse.mm(A0, torch.zeros((K, 8), device=dev), red)
        torch.cuda.synchronize()
        sparse_mm = "ok"
    except Exception as e:   # noqa: BLE001 (the message is the record)
        sparse_mm = "%s: %s" % (type(e).__name__, str(e).split("\n")[0][:200])

    def composition(B):
        P = vleaf[:, None] * B[col64]          # (nnz, N), materialised
        if args.composition == "segment":
            return torch.segment_reduce(P, "max" if red == "amax" else "min", lengths=lens, axis=0)
        out = torch.zeros((M, B.shape[1]), dtype=P.dtype, device=dev)
        return out.scatter_reduce(0, row[:, None].expand(-1, B.shape[1]), P, red, include_self=False)

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / reps   # us per call

    def stats(ts):
        med = statistics.median(ts)
        return {"median_us": med, "min_us": min(ts), "max_us": max(ts), "spread": (max(ts) - min(ts)) / med}

    def compare(f, c):
        r = {"fused": stats(f), "composition": stats(c)}
        r["ratio"] = r["composition"]["median_us"] / r["fused"]["median_us"]
        r["verdict"] = "fused" if max(f) < min(c) else "composition" if max(c) < min(f) else "undecided"
        return r

    for N in [int(t) for t in args.dims.split(",") if t]:
        B = (torch.rand((K, N), device=dev, generator=gen) * 2 - 1).requires_grad_()
        G = torch.rand((M, N), device=dev, generator=gen) * 2 - 1
        leaves = (B, A, vleaf) if args.grad_a else (B,)

        def apply(side):
            if side == "fused":
                return torch_op.spmm_reduce(A, B, red)
            if side == "sum":
                return torch_op.spmm(A, B)
            return composition(B)

        def forward(side):
            with torch.no_grad():
                apply(side)

        def step(side):
            for t in leaves:
                t.grad = None
            apply(side).backward(G)

        torch_op.clear_cache()
        rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": int(nnz), "N": N, "reduce": red, "rounds": args.rounds,
               "composition_form": args.composition + "_reduce", "grad_a": bool(args.grad_a), "torch_sparse_mm_gpu": sparse_mm}
        if args.tag:
            rec["tag"] = args.tag
        sides = ["fused"] if args.fused_only else ["fused", "composition"]
        peak = {}
        for side in list(sides) + ["sum"]:   # warm-up, and the peak of one step
            try:
                step(side)
                for t in leaves:
                    t.grad = None
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                base = torch.cuda.memory_allocated(dev)
                step(side)
                torch.cuda.synchronize()
                peak[side] = int(torch.cuda.max_memory_allocated(dev) - base)
            except torch.OutOfMemoryError:
                if side != "composition":
                    raise
                for t in leaves:
                    t.grad = None
                torch.cuda.empty_cache()
                sides.remove("composition")
                rec["composition"] = "out of memory"
        rec["peak_bytes"] = peak
        rec["value_refreshes"] = torch_op.cache_info()["value_refreshes"]
        for name, fn in (("forward", forward), ("forward_backward", step)):
            once = max(timed(lambda: fn(s), 1) for s in sides)
            reps = int(max(1, min(args.max_reps, args.round_ms * 1e3 / once)))
            ts = {s: [] for s in sides + ["sum"]}
            for _ in range(args.rounds):   # alternating rounds
                for s in ts:
                    ts[s].append(timed(lambda: fn(s), reps))
            rec[name] = compare(ts["fused"], ts["composition"]) if "composition" in ts else {"fused": stats(ts["fused"])}
            rec[name]["spmm_sum"] = stats(ts["sum"])
            rec[name]["reps"] = reps
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        torch_op.clear_cache()
        del B, G, leaves
        torch.cuda.empty_cache()
    if args.out and not args.fused_only:   # per workload: does the fused path beat the composition by more than the spread between repeats?
        with open(args.out) as fh:
            recs = [r for r in map(json.loads, fh) if r["matrix"] == args.matrix]
        for name in ("forward", "forward_backward"):
            verdicts = ["N%d %s" % (r["N"], "%s x%.2f" % (r[name]["verdict"], r[name]["ratio"]) if "verdict" in r[name] else "composition: out of memory")
                        for r in recs]
            print("%s %s: %s" % (args.matrix, name, "; ".join(verdicts)))


if __name__ == "__main__":
    main()
