"""sextans_amd.gated.spmm_gated against the composition a user is left with without it -- z = x_dst[rows] + x_src[cols] (+ E), materialised
as (nnz, N) tensors, torch.sigmoid, torch_op.spmm_edge(A, V, g, "mul"), for the normalised mode torch_op.spmm_edge(A, None, g, "copy") and
a division, autograd through all of it (the gathers' backward is an atomic index_add_) -- on the same commit, the same process and the
same tensors, on one GPU.

    python tools/spmm_gated_bench.py --matrix config4 --out profiles/spmm_gated.jsonl     (appends one record per N, mode and E / no E)
    python tools/spmm_gated_bench.py --matrix small --dims 16,64

Matrices: "config4" = gen_csr_device(4 M, 4 M, Poisson(40)), "fem" = gen_fem3d_device(110, 110, 110, 3) (3.99 M rows, 318 M non-zeros),
"powerlaw" = gen_powerlaw_device(1 M, 1 M, 6, 1.2, 400 000), "small" = a 200 k-row config-4 for trying the tool out.
The composition's 64-bit row and column indices are built once, outside every timed region.  Per record: the forward alone (no autograd
graph) and forward + backward (the gradients of x_dst, x_src, V and, when present, E), each side timed between HIP events over --rounds
rounds of `reps` calls, the sides in ALTERNATING rounds after one untimed warm-up step per side (engine, A^T and tables are built there);
reps is chosen per record so that a round lasts about --round-ms.  "ratio" = composition median / fused median (> 1: the fused path is
faster), "spread" = (max - min) / median of a side's rounds, "verdict": "fused" / "composition" when that side's slowest round beats the
other's fastest -- a difference larger than the spread between repeats -- else "undecided".
"peak_bytes": torch.cuda.max_memory_allocated over one forward + backward step of a side, above what was allocated before it (the
operands, E among them, are allocated before).  A case whose operands or whose composition cannot be allocated is recorded as such
("operands": "out of memory" / "composition": "out of memory"); in the second case the fused side is timed alone."""
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
    ap.add_argument("--modes", default="sum,norm")
    ap.add_argument("--edge", default="0,1", help="0: without E, 1: with E")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-ms", type=float, default=200.0)
    ap.add_argument("--max-reps", type=int, default=8)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from sextans_amd import api, torch_op
    from sextans_amd.gated import spmm_gated
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
    lens = (crow[1:] - crow[:-1]).long()       # built once, untimed
    row64 = torch.repeat_interleave(torch.arange(M, device=dev), lens, output_size=nnz)
    col64 = col.long()
    eps = 1e-6

    def composition(xd, xs, V, E, norm):
        z = xd[row64] + xs[col64]              # (nnz, N), materialised
        if E is not None:
            z = z + E
        g = torch.sigmoid(z)
        num = torch_op.spmm_edge(A, V, g, "mul")
        if not norm:
            return num
        return num / (torch_op.spmm_edge(A, None, g, "copy") + eps)

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

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    cases = [(int(n), m, e == "1") for n in args.dims.split(",") if n for m in args.modes.split(",") if m for e in args.edge.split(",") if e]
    for N, mode, with_e in cases:
        norm = mode == "norm"
        rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "mode": mode, "edge_features": with_e, "rounds": args.rounds,
               "composition_form": "gathers, sigmoid, spmm_edge mul" + (", spmm_edge copy, division" if norm else ""),
               "grads": "x_dst, x_src, V" + (", E" if with_e else "")}
        torch_op.clear_cache()
        try:
            rand = lambda rows: (torch.rand((rows, N), device=dev, generator=gen) * 2 - 1)   # noqa: E731
            xd, xs, V = rand(M).requires_grad_(), rand(K).requires_grad_(), rand(K).requires_grad_()
            E = rand(nnz).requires_grad_() if with_e else None
            G = rand(M)
        except torch.OutOfMemoryError:
            xd = xs = V = E = G = None
            torch.cuda.empty_cache()
            rec["operands"] = "out of memory"
            emit(rec)
            continue
        leaves = [t for t in (xd, xs, V, E) if t is not None]

        def apply(side):
            if side == "fused":
                return spmm_gated(A, xd, xs, V, E, normalize=norm, eps=eps)
            return composition(xd, xs, V, E, norm)

        def forward(side):
            with torch.no_grad():
                apply(side)

        def step(side):
            for x in leaves:
                x.grad = None
            apply(side).backward(G)

        sides = ["fused", "composition"]
        peak = {}
        for side in list(sides):   # warm-up, and the peak of one step
            try:
                step(side)
                for x in leaves:
                    x.grad = None
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                base = torch.cuda.memory_allocated(dev)
                step(side)
                torch.cuda.synchronize()
                peak[side] = int(torch.cuda.max_memory_allocated(dev) - base)
            except torch.OutOfMemoryError:
                if side != "composition":
                    raise
                for x in leaves:
                    x.grad = None
                torch.cuda.empty_cache()
                sides.remove("composition")
                rec["composition"] = "out of memory"
        rec["peak_bytes"] = peak
        rec["value_refreshes"] = torch_op.cache_info()["value_refreshes"]
        for name, fn in (("forward", forward), ("forward_backward", step)):
            for x in leaves:
                x.grad = None
            try:
                once = max(timed(lambda: fn(s), 1) for s in sides)
            except torch.OutOfMemoryError:   # (the forward alone fitted, or the other way round)
                torch.cuda.empty_cache()
                sides.remove("composition")
                rec["composition"] = "out of memory"
                once = timed(lambda: fn("fused"), 1)
            reps = int(max(1, min(args.max_reps, args.round_ms * 1e3 / once)))
            ts = {s: [] for s in sides}
            for _ in range(args.rounds):   # alternating rounds
                for s in ts:
                    ts[s].append(timed(lambda: fn(s), reps))
            rec[name] = compare(ts["fused"], ts["composition"]) if "composition" in ts else {"fused": stats(ts["fused"])}
            rec[name]["reps"] = reps
        emit(rec)
        torch_op.clear_cache()
        del xd, xs, V, E, G, leaves
        torch.cuda.empty_cache()
    if args.out:   # per workload: does the fused path beat the composition by more than the spread between repeats?
        with open(args.out) as fh:
            recs = [r for r in map(json.loads, fh) if r["matrix"] == args.matrix and "forward" in r]
        for name in ("forward", "forward_backward"):
            verdicts = ["N%d %s%s %s" % (r["N"], r["mode"], "+E" if r["edge_features"] else "",
                                         "%s x%.2f" % (r[name]["verdict"], r[name]["ratio"]) if "verdict" in r[name] else "composition: out of memory")
                        for r in recs]
            print("%s %s: %s" % (args.matrix, name, "; ".join(verdicts)))


if __name__ == "__main__":
    main()
