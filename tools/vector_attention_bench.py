"""vector_attention.vector_attention(A, S, V, D) against the composition torch allows on a GPU -- materialise the (nnz, N) messages
(V[col] for "node", V[col] + D for "add"), then torch.segment_reduce max of the scores S over the row lengths, exp, segment_reduce sum,
the weighted segment_reduce sum, autograd through it -- on the same commit, the same process and the same tensors, on one GPU.

    python tools/vector_attention_bench.py --matrix config4 --out profiles/vector_attention.jsonl     (appends one record per N and mode)
    python tools/vector_attention_bench.py --matrix small --dims 16,64 --modes node,add

Matrices: "config4" = gen_csr_device(4 M, 4 M, Poisson(40)), "fem" = gen_fem3d_device(110, 110, 110, 3) (3.99 M rows, 318 M non-zeros),
"powerlaw" = gen_powerlaw_device(1 M, 1 M, 6, 1.2, 400 000), "small" = a 200 k-row config-4 for trying the tool out: the matrices of
tools/spmm_edge_softagg_bench.py.
The composition's row lengths and 64-bit column indices are built once, outside every timed region.  Per N and mode: the forward alone
(no autograd graph) and forward + backward (the gradients of S, of V and -- "add" -- of D), each side timed between HIP events over
--rounds rounds of `reps` calls, the sides in ALTERNATING rounds after one untimed warm-up step per side (engine, A^T and tables are
built there); reps is chosen per record so that a round lasts about --round-ms.  "ratio" = composition median / fused median (> 1: the
fused path is faster), "spread" = (max - min) / median of a side's rounds, "verdict": "fused" / "composition" when that side's slowest
round beats the other's fastest -- a difference larger than the spread between repeats -- else "undecided".
"peak_bytes": torch.cuda.max_memory_allocated over one forward + backward step of a side, above what was allocated before it (S, V, D,
G and the matrix are allocated before it on every side).  A composition case that cannot be allocated is recorded as such
("composition": "out of memory") and the fused side is timed alone; operands that cannot be allocated end the record
("operands": "out of memory"), and so does a fused training step whose gradients do not fit next to them ("fused": "out of memory").
For information, on the same matrix and N, the sibling without the S stream: "spmm_edge_softagg" = edge_softagg.spmm_edge_softagg(A, V,
D, "add") for "add" (the same messages, the score computed from them: what reading S and writing dS cost), "spmm_softagg" =
torch_op.spmm_softagg(A, V) for "node" (the messages val[e] * V[c]).
"bytes_per_entry": what the fused forward must at least move per stored entry (4 + 8 N: the column index, the S row and a gathered V
row; 4 + 12 N for "add", which reads the D row as well), for reading the times against.
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
    ap.add_argument("--modes", default="node,add")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-ms", type=float, default=200.0)
    ap.add_argument("--max-reps", type=int, default=8)
    ap.add_argument("--tag", default="", help="written into every record as \"tag\" (names the build that was timed)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from sextans_amd import api, torch_op
    from sextans_amd.edge_softagg import spmm_edge_softagg
    from sextans_amd.vector_attention import vector_attention
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

    def composition(S, V, D):
        P = V[col64] if D is None else V[col64] + D   # (nnz, N) messages, materialised
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

    def uniform(rows, N, scale):
        return torch.rand((rows, N), device=dev, generator=gen).mul_(2 * scale).sub_(scale)

    for N in [int(x) for x in args.dims.split(",") if x]:
        for mode in [x for x in args.modes.split(",") if x]:
            S = V = D = G = None
            try:
                V = uniform(K, N, 1.0).requires_grad_()
                G = uniform(M, N, 1.0)
                S = uniform(nnz, N, 4.0).requires_grad_()          # scores in [-4, 4)
                D = uniform(nnz, N, 1.0).requires_grad_() if mode == "add" else None
            except torch.OutOfMemoryError:
                del S, V, D, G
                torch.cuda.empty_cache()
                emit({"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "mode": mode, "operands": "out of memory",
                      "operand_bytes": 4 * N * (K + M + nnz * (2 if mode == "add" else 1))})
                continue
            leaves = [x for x in (S, V, D) if x is not None]
            extra = "spmm_edge_softagg" if mode == "add" else "spmm_softagg"

            def apply(side):
                if side == "fused":
                    return vector_attention(A, S, V, D)
                if side == "spmm_edge_softagg":
                    return spmm_edge_softagg(A, V, D, op="add")
                if side == "spmm_softagg":
                    return torch_op.spmm_softagg(A, V)
                return composition(S, V, D)

            def forward(side):
                with torch.no_grad():
                    apply(side)

            def step(side):
                for x in leaves:
                    x.grad = None
                apply(side).backward(G)

            torch_op.clear_cache()
            rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "mode": mode, "rounds": args.rounds,
                   "composition_form": "messages materialised, segment_reduce max, exp, sum, weighted sum",
                   "grads": ", ".join(("S", "V", "D") if mode == "add" else ("S", "V")),
                   "bytes_per_entry": {"fused_forward_at_least": 4 + (12 if mode == "add" else 8) * N}}
            if args.tag:
                rec["tag"] = args.tag
            sides = ["fused", "composition"]
            extras = [extra]
            peak = {}
            for side in list(sides) + extras:   # warm-up, and the peak of one step
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
                    if side in sides:
                        sides.remove(side)
                    else:
                        extras.remove(side)
                    rec[side] = "out of memory"
                for x in leaves:
                    x.grad = None
                torch.cuda.empty_cache()
                if "fused" not in sides:   # (the gradients of a training step do not fit next to the operands: nothing to compare)
                    break
            rec["peak_bytes"] = peak
            if "fused" not in sides:
                emit(rec)
                torch_op.clear_cache()
                del S, V, D, G, leaves
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
                ts = {s: [] for s in sides + extras}
                for _ in range(args.rounds):   # alternating rounds
                    for s in ts:
                        ts[s].append(timed(lambda: fn(s), reps))
                rec[name] = compare(ts["fused"], ts["composition"]) if "composition" in ts else {"fused": stats(ts["fused"])}
                for s in extras:
                    rec[name][s] = stats(ts[s])
                rec[name]["reps"] = reps
                for x in leaves:
                    x.grad = None
                torch.cuda.empty_cache()
            emit(rec)
            torch_op.clear_cache()
            del S, V, D, G, leaves
            torch.cuda.empty_cache()
    if args.out:   # per workload: does the fused path beat the composition by more than the spread between repeats?
        with open(args.out) as fh:
            recs = [r for r in map(json.loads, fh) if r["matrix"] == args.matrix and "forward" in r]
        for name in ("forward", "forward_backward"):
            verdicts = ["N%d %s %s" % (r["N"], r["mode"], "%s x%.2f" % (r[name]["verdict"], r[name]["ratio"]) if "verdict" in r[name]
                                       else "composition: out of memory") for r in recs]
            print("%s %s: %s" % (args.matrix, name, "; ".join(verdicts)))


if __name__ == "__main__":
    main()
