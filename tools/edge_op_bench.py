"""edge_op.edge_op(A, x_dst, x_src, E, op) against the composition torch allows on a GPU -- x_dst[rows] (op) x_src[cols] (+ E) with the
gathers by torch_op.entry_rows(A) and A.col_indices() as 64-bit indices, autograd through index_add_ (float atomics) -- in the same
process on the same tensors, on one GPU.  The composition calls nothing of this library inside its timed region, so it is what the parent
commit offers.

    python tools/edge_op_bench.py --matrix config4 --out profiles/edge_op.jsonl     (appends one record per N and case)
    python tools/edge_op_bench.py --matrix small --dims 16,64 --cases add,add_e,mul

Matrices: "config4" = gen_csr_device(4 M, 4 M, Poisson(40)), "fem" = gen_fem3d_device(110, 110, 110, 3) (3.99 M rows, 318 M non-zeros),
"powerlaw" = gen_powerlaw_device(1 M, 1 M, 6, 1.2, 400 000), "small" = a 200 k-row config-4 for trying the tool out: the matrices of
tools/vector_attention_bench.py.  Cases: "add" (no E), "add_e" (with E), "mul" (no E).
The composition's 64-bit row and column indices are built once, outside every timed region.  Per N and case: the forward alone (no
autograd graph) and forward + backward (the gradients of x_dst, x_src and -- "add_e" -- E), each side timed between HIP events over
--rounds rounds of `reps` calls, the sides in ALTERNATING rounds after one untimed warm-up step per side (engine, A^T and tables are
built there); reps is chosen per record so that a round lasts about --round-ms.  "ratio" = composition median / fused median (> 1: the
fused path is faster), "spread" = (max - min) / median of a side's rounds, "verdict": "fused" / "composition" when that side's slowest
round beats the other's fastest -- a difference larger than the spread between repeats -- else "undecided" (DESIGN 4.12).
"peak_bytes": torch.cuda.max_memory_allocated over one forward + backward step of a side, above what was allocated before it (the
operands, the upstream gradient and the matrix are allocated before it on every side).  A composition case that cannot be allocated is
recorded as such ("composition": "out of memory") and the fused side is timed alone; operands that cannot be allocated end the record.
"bytes_per_entry": what each forward must at least move per stored entry -- fused: the 4-byte column index, a gathered x_src row and
the Z row (4 + 8 N; + 4 N with E; the x_dst row is read once per row); composition: two 8-byte indices, each gather's read and write,
the elementwise pass's two reads and one write (16 + 28 N; + 12 N with E).
--tag NAME is written into every record and says which build it timed."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"add": ("add", False), "add_e": ("add", True), "mul": ("mul", False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", choices=["config4", "fem", "powerlaw", "small"], default="small")
    ap.add_argument("--dims", default="16,64")
    ap.add_argument("--cases", default="add,add_e,mul")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-ms", type=float, default=200.0)
    ap.add_argument("--max-reps", type=int, default=8)
    ap.add_argument("--tag", default="", help="written into every record as \"tag\" (names the build that was timed)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from sextans_amd import api, torch_op
    from sextans_amd.edge_op import edge_op
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
    rows64 = torch_op.entry_rows(A)            # built once, untimed
    col64 = col.long()

    def composition(op, xd, xs, E):
        d, s = xd[rows64], xs[col64]           # two (nnz, N) gathers, materialised
        z = d + s if op == "add" else d * s
        return z + E if E is not None else z

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

    def uniform(rows, N):
        return torch.rand((rows, N), device=dev, generator=gen).mul_(2.0).sub_(1.0)

    for N in [int(x) for x in args.dims.split(",") if x]:
        for case in [x for x in args.cases.split(",") if x]:
            op, with_e = CASES[case]
            xd = xs = E = G = None
            try:
                xd, xs = uniform(M, N).requires_grad_(), uniform(K, N).requires_grad_()
                G = uniform(nnz, N)
                E = uniform(nnz, N).requires_grad_() if with_e else None
            except torch.OutOfMemoryError:
                del xd, xs, E, G
                torch.cuda.empty_cache()
                emit({"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "case": case, "operands": "out of memory",
                      "operand_bytes": 4 * N * (K + M + nnz * (2 if with_e else 1))})
                continue
            leaves = [x for x in (xd, xs, E) if x is not None]

            def apply(side):
                return edge_op(A, xd, xs, E, op=op) if side == "fused" else composition(op, xd, xs, E)

            def forward(side):
                with torch.no_grad():
                    apply(side)

            def step(side):
                for x in leaves:
                    x.grad = None
                apply(side).backward(G)

            torch_op.clear_cache()
            rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "case": case, "rounds": args.rounds,
                   "composition_form": "x_dst[entry_rows] op x_src[col_indices] (+ E), int64 indices, autograd through index_add_",
                   "grads": ", ".join(("x_dst", "x_src", "E") if with_e else ("x_dst", "x_src")),
                   "bytes_per_entry": {"fused_forward_at_least": 4 + (12 if with_e else 8) * N,
                                       "composition_forward_at_least": 16 + (40 if with_e else 28) * N}}
            if args.tag:
                rec["tag"] = args.tag
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
                    sides.remove(side)
                    rec[side] = "out of memory"
                for x in leaves:
                    x.grad = None
                torch.cuda.empty_cache()
                if "fused" not in sides:   # (a training step does not fit next to the operands: nothing to compare)
                    break
            rec["peak_bytes"] = peak
            if "fused" not in sides:
                emit(rec)
                torch_op.clear_cache()
                del xd, xs, E, G, leaves
                torch.cuda.empty_cache()
                continue
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
                ts = {s: [] for s in sides}
                for _ in range(args.rounds):   # alternating rounds
                    for s in ts:
                        ts[s].append(timed(lambda: fn(s), reps))
                rec[name] = compare(ts["fused"], ts["composition"]) if "composition" in ts else {"fused": stats(ts["fused"])}
                rec[name]["reps"] = reps
                for x in leaves:
                    x.grad = None
                torch.cuda.empty_cache()
            emit(rec)
            torch_op.clear_cache()
            del xd, xs, E, G, leaves
            torch.cuda.empty_cache()
    if args.out:   # per workload: does the fused path beat the composition by more than the spread between repeats?
        with open(args.out) as fh:
            recs = [r for r in map(json.loads, fh) if r["matrix"] == args.matrix and "forward" in r]
        for name in ("forward", "forward_backward"):
            verdicts = ["N%d %s %s" % (r["N"], r["case"], "%s x%.2f" % (r[name]["verdict"], r[name]["ratio"]) if "verdict" in r[name]
                                       else "composition: out of memory") for r in recs]
            print("%s %s: %s" % (args.matrix, name, "; ".join(verdicts)))


if __name__ == "__main__":
    main()
