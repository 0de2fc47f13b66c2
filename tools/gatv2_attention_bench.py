"""gatv2_attention against the composition a user can write with the other ops of torch_op -- materialise x_dst[row] + x_src[col] as an
(nnz, H, d) tensor, leaky_relu, multiply by att and sum over d, then row_softmax and spmm once per head, stacked -- on the same commit, the
same process and the same tensors, on one GPU.

    python tools/gatv2_attention_bench.py --matrix config4 --out profiles/gatv2_attention.jsonl     (appends one record per (H, d))
    python tools/gatv2_attention_bench.py --matrix small --heads 1,8 --dims 16,64

Matrices: "config4" = gen_csr_device(4 M, 4 M, Poisson(40)), "fem" = gen_fem3d_device(110, 110, 110, 3) (3.99 M rows, 318 M non-zeros),
"powerlaw" = gen_powerlaw_device(1 M, 1 M, 6, 1.2, 400 000), "small" = a 200 k-row config-4 for trying the tool out.
The composition's nnz-long row-index vector is built once, outside every timed region; its scores become a sparse_csr matrix on A's
index tensors through a small autograd function of the tool's (torch's constructor differentiates through a dense matrix).  Per (H, d):
the forward alone (no autograd graph) and forward + backward (gradients of x_dst, x_src and att), each side timed between HIP events over
--rounds rounds of `reps` calls, the two sides in ALTERNATING rounds after one untimed warm-up step per side (engine, A^T, plans and
tables are built there); reps is chosen per record so that a round lasts about --round-ms.  "ratio" = composition median / fused median
(> 1: the fused path is faster), "spread" = (max - min) / median of a side's rounds, "verdict": "fused" / "composition" when that side's
slowest round beats the other's fastest -- a difference larger than the spread between repeats -- else "undecided".
"peak_bytes": torch.cuda.max_memory_allocated over one forward + backward step of a side, above what was allocated before it.
A composition case that cannot be allocated is recorded as such ("composition": "out of memory", with the bytes of ONE (nnz, H, d) fp32
tensor as "composition_edge_tensor_bytes") and the fused side is timed alone.
--fused-only times gatv2_attention alone (for choosing the kernels' entries-in-flight count between two builds, or under a profiler): no
composition, no verdict; --tag NAME is written into every record and says which build it timed."""
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
    ap.add_argument("--heads", default="1,8")
    ap.add_argument("--dims", default="16,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-ms", type=float, default=200.0)
    ap.add_argument("--max-reps", type=int, default=8)
    ap.add_argument("--slope", type=float, default=0.2)
    ap.add_argument("--fused-only", action="store_true", help="time gatv2_attention alone (kernel tuning, profiling): no composition, no verdict")
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
    gen = torch.Generator(device=dev).manual_seed(1)
    row = torch.repeat_interleave(torch.arange(M, device=dev), (crow[1:] - crow[:-1]).long(), output_size=int(nnz))   # built once, untimed
    col64 = col.long()

    class OnPattern(torch.autograd.Function):
        """nnz values -> the sparse_csr matrix on A's index tensors; the gradient is the CSR gradient's values.  (The backward of torch's own
        constructor goes through a dense M x K tensor: not an option at these sizes, so the composition carries these ten lines.)"""

        @staticmethod
        def forward(ctx, values):
            return torch.sparse_csr_tensor(crow, col, values, size=(M, K))

        @staticmethod
        def backward(ctx, g):
            return g.values()

    def composition(xd, xs, att):
        s = (torch.nn.functional.leaky_relu(xd[row] + xs[col64], args.slope) * att).sum(-1)   # (nnz, H, d) materialised, -> (nnz, H)
        outs = []
        for h in range(xs.shape[1]):
            P = torch_op.row_softmax(OnPattern.apply(s[:, h].contiguous()))
            outs.append(torch_op.spmm(P, xs[:, h]))
        return torch.stack(outs, dim=1)

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

    for H in [int(t) for t in args.heads.split(",") if t]:
        for d in [int(t) for t in args.dims.split(",") if t]:
            xd, xs = (((torch.rand((n, H, d), device=dev, generator=gen) * 2 - 1) * 0.5).requires_grad_() for n in (M, K))
            att = ((torch.rand((H, d), device=dev, generator=gen) * 2 - 1) * 0.5).requires_grad_()
            G = torch.rand((M, H, d), device=dev, generator=gen) * 2 - 1
            params = (xd, xs, att)

            def apply(side):
                return torch_op.gatv2_attention(A, xd, xs, att, negative_slope=args.slope) if side == "fused" else composition(xd, xs, att)

            def forward(side):
                with torch.no_grad():
                    apply(side)

            def step(side):
                for t in params:
                    t.grad = None
                apply(side).backward(G)

            torch_op.clear_cache()
            rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": int(nnz), "H": H, "d": d, "slope": args.slope, "rounds": args.rounds}
            if args.tag:
                rec["tag"] = args.tag
            sides = ["fused"] if args.fused_only else ["fused", "composition"]
            peak = {}
            for side in list(sides):   # warm-up, and the peak of one step
                try:
                    step(side)
                    for t in params:
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
                    for t in params:
                        t.grad = None
                    torch.cuda.empty_cache()
                    sides.remove("composition")
                    rec["composition"] = "out of memory"
                    rec["composition_edge_tensor_bytes"] = int(nnz) * H * d * 4
            rec["peak_bytes"] = peak
            rec["value_refreshes_composition"] = torch_op.cache_info()["value_refreshes"]
            for name, fn in (("forward", forward), ("forward_backward", step)):
                once = max(timed(lambda: fn(s), 1) for s in sides)
                reps = int(max(1, min(args.max_reps, args.round_ms * 1e3 / once)))
                ts = {s: [] for s in sides}
                for _ in range(args.rounds):   # alternating rounds
                    for s in ts:
                        ts[s].append(timed(lambda: fn(s), reps))
                rec[name] = compare(ts["fused"], ts["composition"]) if "composition" in ts else {"fused": stats(ts["fused"])}
                rec[name]["reps"] = reps
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as fh:
                    fh.write(line + "\n")
            torch_op.clear_cache()
            del xd, xs, att, G, params
            torch.cuda.empty_cache()
    if args.out and not args.fused_only:   # per workload: does the fused path beat the composition by more than the spread between repeats?
        with open(args.out) as fh:
            recs = [r for r in map(json.loads, fh) if r["matrix"] == args.matrix]
        for name in ("forward", "forward_backward"):
            verdicts = ["H%d d%d %s" % (r["H"], r["d"], "%s x%.2f" % (r[name]["verdict"], r[name]["ratio"]) if "verdict" in r[name]
                                        else "composition: out of memory") for r in recs]
            print("%s %s: %s" % (args.matrix, name, "; ".join(verdicts)))


if __name__ == "__main__":
    main()
