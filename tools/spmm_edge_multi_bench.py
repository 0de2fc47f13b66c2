"""spmm_edge_multi(A, B, E, op, aggr) against the composition available on the same commit, in the same process and on the same tensors,
on one GPU: the messages materialised by torch (m = E for "copy", B[col] * E for "mul"), spmm_edge(A, None, m, "copy") for the sum,
spmm_edge(A, None, m * m, "copy") for the sum of squares, torch.segment_reduce(m, "max" / "min", offsets=crow) for the extrema -- those of
them the aggregate set needs --, the same elementwise mean / var / std formulas on top, and autograd through all of it.

    python tools/spmm_edge_multi_bench.py --matrix config4 --out profiles/spmm_edge_multi.jsonl   (appends one record per N, op and set)
    python tools/spmm_edge_multi_bench.py --matrix small --dims 16,64

Matrices: "config4" = gen_csr_device(4 M, 4 M, Poisson(40)), "fem" = gen_fem3d_device(110, 110, 110, 3) (3.99 M rows, 318 M non-zeros),
"powerlaw" = gen_powerlaw_device(1 M, 1 M, 6, 1.2, 400 000), "small" = a 200 k-row config-4 for trying the tool out.
Per N, op ("copy", "mul") and aggregate set ("mean,max,min,std" and "max"): the forward alone (no autograd graph) and forward + backward
(the gradients of E and, for "mul", of B), each side timed between HIP events over --rounds rounds of `reps` calls, the two sides in
ALTERNATING rounds after one untimed warm-up step per side (engines, A^T and tables are built there); reps is chosen per record so that
a round lasts about --round-ms.  "ratio" = composition median / fused median (> 1: the fused path is faster), "spread" = (max - min) /
median of a side's rounds, "verdict": "fused" / "composition" when that side's slowest round beats the other's fastest -- a difference
larger than the spread between repeats -- else "undecided".  "peak_bytes": torch.cuda.max_memory_allocated over one forward + backward
step of a side, above what was allocated before it (E and B are allocated before it).  A side that cannot be allocated is recorded as
{"error": "out of memory"} and the record carries no verdict.  "max_abs_diff": fused against composition over the rows that hold an
entry (torch.segment_reduce gives an empty row -inf / +inf, the fused op 0)."""
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
    ap.add_argument("--ops", default="copy,mul")
    ap.add_argument("--aggr", default="mean,max,min,std;max", help="aggregate sets, ';' between sets")
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
    crow = torch.empty(M + 1, dtype=torch.int32, device=dev); col = torch.empty(nnz, dtype=torch.int32, device=dev)
    for dst, src, n in ((crow, p, (M + 1) * 4), (col, i, nnz * 4)):
        api.device_copy(0, dst.data_ptr(), src, n)
    for src in (p, i, v):
        api.device_free(0, src)
    A = torch.sparse_csr_tensor(crow, col, torch.ones(nnz, dtype=torch.float32, device=dev), size=(M, K))   # (only the pattern is used)
    offsets, col64 = crow.to(torch.int64), col.to(torch.int64)     # what the composition's torch ops index with
    lens = crow[1:] - crow[:-1]
    deg = lens.clamp(min=1).to(torch.float32)[:, None]
    nonempty = lens > 0
    gen = torch.Generator(device=dev).manual_seed(1)
    eps = 1e-5

    def composition(B, E, op, aggr):
        m = E if op == "copy" else B[col64] * E
        raw = {}
        if any(x in aggr for x in ("sum", "mean", "var", "std")):
            raw["sum"] = torch_op.spmm_edge(A, None, m, "copy")
        if any(x in aggr for x in ("sumsq", "var", "std")):
            raw["sumsq"] = torch_op.spmm_edge(A, None, m * m, "copy")
        if "max" in aggr:
            raw["max"] = torch.segment_reduce(m, "max", offsets=offsets, axis=0)
        if "min" in aggr:
            raw["min"] = torch.segment_reduce(m, "min", offsets=offsets, axis=0)
        if "sum" in raw:
            raw["mean"] = raw["sum"] / deg
        if "sumsq" in raw:
            raw["var"] = raw["sumsq"] / deg - raw["mean"] ** 2
            raw["std"] = torch.sqrt(torch.relu(raw["var"]) + eps)
        return torch.cat([raw[x] for x in aggr], dim=1) if len(aggr) > 1 else raw[aggr[0]]

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

    for N in [int(t) for t in args.dims.split(",") if t]:
        for op in [t for t in args.ops.split(",") if t]:
            for aggr in [tuple(s.split(",")) for s in args.aggr.split(";") if s]:
                rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": int(nnz), "N": N, "op": op, "aggr": list(aggr), "rounds": args.rounds,
                       "composition_form": "torch messages + spmm_edge(copy) x2 + segment_reduce x2"}
                if args.tag:
                    rec["tag"] = args.tag
                torch_op.clear_cache()
                B = E = G = None
                try:
                    E = (torch.rand((nnz, N), device=dev, generator=gen) * 2 - 1).requires_grad_()
                    B = (torch.rand((K, N), device=dev, generator=gen) * 2 - 1).requires_grad_() if op != "copy" else None
                    G = torch.rand((M, len(aggr) * N), device=dev, generator=gen) * 2 - 1
                except torch.cuda.OutOfMemoryError:
                    rec["error"] = "out of memory: the operands (E is nnz x N floats)"
                    emit(rec)
                    del B, E, G
                    torch.cuda.empty_cache()
                    continue

                def apply(side):
                    if side == "fused":
                        return torch_op.spmm_edge_multi(A, B, E, op, aggr, eps=eps)
                    return composition(B, E, op, aggr)

                def forward(side):
                    with torch.no_grad():
                        apply(side)

                def step(side):
                    E.grad = None
                    if B is not None:
                        B.grad = None
                    apply(side).backward(G)

                sides = ["fused", "composition"]
                peak, failed = {}, set()
                for side in sides:   # warm-up, and the peak of one step
                    try:
                        step(side)
                        E.grad = None
                        if B is not None:
                            B.grad = None
                        torch.cuda.synchronize()
                        torch.cuda.reset_peak_memory_stats(dev)
                        base = torch.cuda.memory_allocated(dev)
                        step(side)
                        torch.cuda.synchronize()
                        peak[side] = int(torch.cuda.max_memory_allocated(dev) - base)
                    except torch.cuda.OutOfMemoryError:
                        failed.add(side)
                        peak[side] = {"error": "out of memory"}
                    E.grad = None
                    if B is not None:
                        B.grad = None
                    torch.cuda.empty_cache()
                rec["peak_bytes"] = peak
                rec["value_refreshes"] = torch_op.cache_info()["value_refreshes"]
                live = [s for s in sides if s not in failed]
                if len(live) == 2:
                    with torch.no_grad():   # the two sides compute the same thing
                        rec["max_abs_diff"] = (apply("fused") - apply("composition"))[nonempty].abs().max().item()
                for name, fn in (("forward", forward), ("forward_backward", step)):
                    if not live:
                        break
                    once = max(timed(lambda: fn(s), 1) for s in live)
                    reps = int(max(1, min(args.max_reps, args.round_ms * 1e3 / once)))
                    ts = {s: [] for s in live}
                    for _ in range(args.rounds):   # alternating rounds
                        for s in ts:
                            ts[s].append(timed(lambda: fn(s), reps))
                    rec[name] = compare(ts["fused"], ts["composition"]) if len(live) == 2 else {live[0]: stats(ts[live[0]])}
                    rec[name]["reps"] = reps
                emit(rec)
                torch_op.clear_cache()
                del B, E, G
                torch.cuda.empty_cache()
    if args.out:   # per workload: does the fused path beat the composition by more than the spread between repeats?
        with open(args.out) as fh:
            recs = [r for r in map(json.loads, fh) if r["matrix"] == args.matrix]
        for name in ("forward", "forward_backward"):
            verdicts = ["N%d %s %s %s" % (r["N"], r["op"], "+".join(r["aggr"]),
                                          "%s x%.2f" % (r[name]["verdict"], r[name]["ratio"]) if "verdict" in r.get(name, {}) else "not allocated")
                        for r in recs]
            print("%s %s: %s" % (args.matrix, name, "; ".join(verdicts)))


if __name__ == "__main__":
    main()
