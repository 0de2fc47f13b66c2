"""spmm_edge(A, B, E, "mul") against the compositions torch allows on a GPU -- gather B[col], multiply with E into a second (nnz, N)
tensor, then reduce it over the rows with torch.segment_reduce (over the row lengths) or with index_add_ (over the row index: float
atomics), autograd through it -- on the same commit, the same process and the same tensors, on one GPU.

    python tools/spmm_edge_bench.py --matrix config4 --out profiles/spmm_edge.jsonl     (appends one record per N)
    python tools/spmm_edge_bench.py --matrix small --dims 16,64

Matrices: "config4" = gen_csr_device(4 M, 4 M, Poisson(40)), "fem" = gen_fem3d_device(110, 110, 110, 3) (3.99 M rows, 318 M non-zeros),
"powerlaw" = gen_powerlaw_device(1 M, 1 M, 6, 1.2, 400 000), "small" = a 200 k-row config-4 for trying the tool out.
The compositions' nnz-long row-index vector (and the row lengths) are built once, outside every timed region.  Per N: the forward alone
(no autograd graph) and forward + backward (the gradients of B and E), each side timed between HIP events over --rounds rounds of
`reps` calls, the sides in ALTERNATING rounds after one untimed warm-up step per side (engine, A^T and tables are built there); reps is
chosen per record so that a round lasts about --round-ms.  Per composition form ("segment_reduce", "index_add"): "ratio" = its median
/ the fused median (> 1: the fused path is faster), "verdict": "fused" / "composition" when that side's slowest round beats the
other's fastest -- a difference larger than the spread between repeats -- else "undecided".  "spread" = (max - min) / median of a
side's rounds.  "peak_bytes": torch.cuda.max_memory_allocated over one forward + backward step of a side, above what was allocated
before it (B, E, G and the matrix are allocated before it on every side).  A composition that cannot be allocated is recorded as
"out of memory" and the other sides are timed without it.  "bytes_per_entry": the traffic the byte count of DESIGN 4.15 expects of the
fused forward (4 + 8 N) and at least of the composition (4 + 16 N), for reading the times against."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = ("segment_reduce", "index_add")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", choices=["config4", "fem", "powerlaw", "small"], default="small")
    ap.add_argument("--dims", default="16,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-ms", type=float, default=200.0)
    ap.add_argument("--max-reps", type=int, default=8)
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
    nnz = int(nnz)
    crow = torch.empty(M + 1, dtype=torch.int32, device=dev); col = torch.empty(nnz, dtype=torch.int32, device=dev)
    val = torch.empty(nnz, dtype=torch.float32, device=dev)
    for dst, src, n in ((crow, p, (M + 1) * 4), (col, i, nnz * 4), (val, v, nnz * 4)):
        api.device_copy(0, dst.data_ptr(), src, n)
        api.device_free(0, src)
    A = torch.sparse_csr_tensor(crow, col, val, size=(M, K))
    gen = torch.Generator(device=dev).manual_seed(1)
    lens = (crow[1:] - crow[:-1]).long()
    row = torch.repeat_interleave(torch.arange(M, device=dev), lens, output_size=nnz)   # built once, untimed
    col64 = col.long()

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
        r = stats(c)
        r["ratio"] = r["median_us"] / statistics.median(f)
        r["verdict"] = "fused" if max(f) < min(c) else "composition" if max(c) < min(f) else "undecided"
        return r

    for N in [int(t) for t in args.dims.split(",") if t]:
        B = (torch.rand((K, N), device=dev, generator=gen) * 2 - 1).requires_grad_()
        E = torch.rand((nnz, N), device=dev, generator=gen).mul_(2).sub_(1).requires_grad_()
        G = torch.rand((M, N), device=dev, generator=gen) * 2 - 1
        leaves = (B, E)

        def apply(side):
            if side == "fused":
                return torch_op.spmm_edge(A, B, E, "mul")
            P = B[col64] * E                       # two (nnz, N) tensors, materialised
            if side == "segment_reduce":
                return torch.segment_reduce(P, "sum", lengths=lens, axis=0)
            return torch.zeros((M, N), dtype=P.dtype, device=dev).index_add_(0, row, P)

        def forward(side):
            with torch.no_grad():
                apply(side)

        def step(side):
            for t in leaves:
                t.grad = None
            apply(side).backward(G)

        torch_op.clear_cache()
        rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "op": "mul", "rounds": args.rounds,
               "bytes_per_entry": {"fused_forward": 4 + 8 * N, "composition_forward_at_least": 4 + 16 * N}}
        if args.tag:
            rec["tag"] = args.tag
        sides = ["fused"] + list(FORMS)
        peak = {}
        for side in list(sides):   # warm-up, and the peak of one step
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
            except RuntimeError as e:   # (torch.OutOfMemoryError is one)
                if side == "fused":
                    raise
                sides.remove(side)
                rec[side] = "out of memory" if isinstance(e, torch.OutOfMemoryError) else "%s: %s" % (type(e).__name__, str(e).split("\n")[0][:200])
            for t in leaves:
                t.grad = None
            torch.cuda.empty_cache()
        rec["peak_bytes"] = peak
        rec["value_refreshes"] = torch_op.cache_info()["value_refreshes"]
        for name, fn in (("forward", forward), ("forward_backward", step)):
            once = max(timed(lambda: fn(s), 1) for s in sides)
            reps = int(max(1, min(args.max_reps, args.round_ms * 1e3 / once)))
            ts = {s: [] for s in sides}
            for _ in range(args.rounds):   # alternating rounds
                for s in ts:
                    ts[s].append(timed(lambda: fn(s), reps))
            rec[name] = {"fused": stats(ts["fused"]), "reps": reps}
            for s in sides[1:]:
                rec[name][s] = compare(ts["fused"], ts[s])
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")
        torch_op.clear_cache()
        del B, E, G, leaves
        torch.cuda.empty_cache()
    if args.out:   # per workload: does the fused path beat each composition by more than the spread between repeats?
        with open(args.out) as fh:
            recs = [r for r in map(json.loads, fh) if r["matrix"] == args.matrix]
        for name in ("forward", "forward_backward"):
            for form in FORMS:
                verdicts = ["N%d %s" % (r["N"], "%s x%.2f" % (r[name][form]["verdict"], r[name][form]["ratio"]) if form in r[name] else r.get(form, "not run"))
                            for r in recs]
                print("%s %s vs %s: %s" % (args.matrix, name, form, "; ".join(verdicts)))


if __name__ == "__main__":
    main()
