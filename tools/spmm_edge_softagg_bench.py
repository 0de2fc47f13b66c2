"""edge_softagg.spmm_edge_softagg(A, B, E, op, t) against the composition torch allows on a GPU -- materialise the (nnz, N) messages
(relu(B[col] + E) for "add_relu", GENConv's; E itself for "copy"), then torch.segment_reduce max of t m over the row lengths, exp,
segment_reduce sum, the weighted segment_reduce sum, autograd through it -- on the same commit, the same process and the same tensors,
on one GPU.

    python tools/spmm_edge_softagg_bench.py --matrix config4 --out profiles/spmm_edge_softagg.jsonl     (appends one record per N and op)
    python tools/spmm_edge_softagg_bench.py --matrix small --dims 16,64 --ops add_relu,copy

Matrices: "config4" = gen_csr_device(4 M, 4 M, Poisson(40)), "fem" = gen_fem3d_device(110, 110, 110, 3) (3.99 M rows, 318 M non-zeros),
"powerlaw" = gen_powerlaw_device(1 M, 1 M, 6, 1.2, 400 000), "small" = a 200 k-row config-4 for trying the tool out.
The composition's row lengths and 64-bit column indices are built once, outside every timed region.  Per N and op: the forward alone (no
autograd graph) and forward + backward (the gradients of B -- not for "copy" --, of E and of the (N,) temperature t), each side timed
between HIP events over --rounds rounds of `reps` calls, the sides in ALTERNATING rounds after one untimed warm-up step per side (engine,
A^T and tables are built there); reps is chosen per record so that a round lasts about --round-ms.  "ratio" = composition median / fused
median (> 1: the fused path is faster), "spread" = (max - min) / median of a side's rounds, "verdict": "fused" / "composition" when that
side's slowest round beats the other's fastest -- a difference larger than the spread between repeats -- else "undecided".
"peak_bytes": torch.cuda.max_memory_allocated over one forward + backward step of a side, above what was allocated before it (B, E, G, t
and the matrix are allocated before it on every side).  A composition case that cannot be allocated is recorded as such
("composition": "out of memory") and the fused side is timed alone; an E that cannot be allocated ends the record ("E": "out of memory").
For information, on the same matrix and N: "spmm_softagg" = torch_op.spmm_softagg(A, B, t), the scalar-weighted messages val[e] * B[c]
under the same softmax (its backward: the gradients of B and t) -- the fused op without the E stream, i.e. what E and dE cost.
"bytes_per_entry": what the fused forward must at least move per stored entry (4 + 8 N: the column index, a gathered B row and the E
row; 4 + 4 N for "copy"), for reading the times against.
--tag NAME is written into every record and says which build it timed."""
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
    ap.add_argument("--ops", default="add_relu,copy")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-ms", type=float, default=200.0)
    ap.add_argument("--max-reps", type=int, default=8)
    ap.add_argument("--tag", default="", help="written into every record as \"tag\" (names the build that was timed)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from sextans_amd import api, torch_op
    from sextans_amd.edge_softagg import spmm_edge_softagg
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
    col64 = col.long()

    def composition(op, B, E, t):
        P = torch.relu(B[col64] + E) if op == "add_relu" else E   # (nnz, N) messages, materialised
        S = P * t
        m = torch.segment_reduce(S.detach(), "max", lengths=lens, axis=0)   # (only a reference point: no gradient through it)
        W = torch.exp(S - torch.repeat_interleave(m, lens, dim=0, output_size=nnz))
        z = torch.segment_reduce(W, "sum", lengths=lens, axis=0)
        acc = torch.segment_reduce(W * P, "sum", lengths=lens, axis=0)
        return acc / z.clamp(min=1e-30)

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

    extras = ["spmm_softagg"]
    for N in [int(x) for x in args.dims.split(",") if x]:
        B = (torch.rand((K, N), device=dev, generator=gen) * 2 - 1).requires_grad_()
        t = (torch.rand((N,), device=dev, generator=gen) * 4 - 1).requires_grad_()   # temperatures in [-1, 3)
        G = torch.rand((M, N), device=dev, generator=gen) * 2 - 1
        try:
            E = torch.rand((nnz, N), device=dev, generator=gen).mul_(2).sub_(1).requires_grad_()
        except torch.OutOfMemoryError:
            torch.cuda.empty_cache()
            emit({"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "E": "out of memory", "E_bytes": 4 * nnz * N})
            continue
        for op in [x for x in args.ops.split(",") if x]:
            leaves = (E, t) if op == "copy" else (B, E, t)

            def apply(side):
                if side == "fused":
                    return spmm_edge_softagg(A, None if op == "copy" else B, E, op=op, t=t)
                if side == "spmm_softagg":
                    return torch_op.spmm_softagg(A, B, t)
                return composition(op, B, E, t)

            def forward(side):
                with torch.no_grad():
                    apply(side)

            def step(side):
                for x in (B, E, t):
                    x.grad = None
                apply(side).backward(G)

            torch_op.clear_cache()
            rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "op": op, "rounds": args.rounds,
                   "composition_form": "messages materialised, segment_reduce max, exp, sum, weighted sum",
                   "grads": ", ".join(("E", "t") if op == "copy" else ("B", "E", "t")),
                   "bytes_per_entry": {"fused_forward_at_least": 4 + (4 if op == "copy" else 8) * N}}
            if args.tag:
                rec["tag"] = args.tag
            sides = ["fused", "composition"]
            peak = {}
            for side in list(sides) + extras:   # warm-up, and the peak of one step
                try:
                    step(side)
                    for x in (B, E, t):
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
                    sides.remove("composition")
                    rec["composition"] = "out of memory"
                for x in (B, E, t):
                    x.grad = None
                torch.cuda.empty_cache()
            rec["peak_bytes"] = peak
            rec["value_refreshes"] = torch_op.cache_info()["value_refreshes"]
            for name, fn in (("forward", forward), ("forward_backward", step)):
                try:
                    once = max(timed(lambda: fn(s), 1) for s in sides)
                except torch.OutOfMemoryError:   # (the step fitted once, or the other way round)
                    torch.cuda.empty_cache()
                    sides.remove("composition")
                    rec["composition"] = "out of memory"
                    once = timed(lambda: fn("fused"), 1)
                reps = int(max(1, min(args.max_reps, args.round_ms * 1e3 / once)))
                ts = {s: [] for s in sides + extras}
                for _ in range(args.rounds):   # alternating rounds
                    for s in ts:
                        ts[s].append(timed(lambda: fn(s), reps))
                rec[name] = compare(ts["fused"], ts["composition"]) if "composition" in ts else {"fused": stats(ts["fused"])}
                for s in extras:
                    rec[name][s] = stats(ts[s])
                rec[name]["reps"] = reps
                for x in (B, E, t):
                    x.grad = None
                torch.cuda.empty_cache()
            emit(rec)
            torch_op.clear_cache()
        del B, E, G, t, leaves
        torch.cuda.empty_cache()
    if args.out:   # per workload: does the fused path beat the composition by more than the spread between repeats?
        with open(args.out) as fh:
            recs = [r for r in map(json.loads, fh) if r["matrix"] == args.matrix and "op" in r]
        for name in ("forward", "forward_backward"):
            verdicts = ["N%d %s %s" % (r["N"], r["op"], "%s x%.2f" % (r[name]["verdict"], r[name]["ratio"]) if "verdict" in r[name]
                                       else "composition: out of memory") for r in recs]
            print("%s %s: %s" % (args.matrix, name, "; ".join(verdicts)))


if __name__ == "__main__":
    main()
