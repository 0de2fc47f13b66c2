"""edge_dot.edge_dot(A, x_dst, x_src) against what the library offered before it, in the same process on the same tensors, on one GPU:
  "sddmm_loop"   torch_op.sddmm once per head on the head's strided slices, .values() stacked to (nnz, H) -- H launches of the same
                 non-zero-dealt algorithm, each re-reading the column indices and the row table; its backward is sddmm's (two SpMMs per
                 head on the gradient's values, value refreshes of the cached engine included);
  "gather"       (x_dst[rows] * x_src[cols]).sum(-1) with the gathers by torch_op.entry_rows(A) and A.col_indices() as 64-bit indices,
                 autograd through index_add_ (float atomics): two (nnz, H, d) temporaries;
  "weight_rows"  FORWARD ONLY: the WEIGHT-mode row pass of sextans_score_attention_backward_device used as a dot product
                 (dS[e, h] = <G[r, h, :], V[c, h, :]> with G := x_dst, V := x_src) -- the ROW-dealt alternative: a hub row is one workgroup
                 per head.  Its FMA chain rounds differently; it is timed, not compared bit for bit.

    python tools/edge_dot_bench.py --matrix config4 --out profiles/edge_dot.jsonl     (appends one record per (H, d))
    python tools/edge_dot_bench.py --matrix small --heads 1,8 --dims 16,64

Matrices: "config4" = gen_csr_device(4 M, 4 M, Poisson(40)), "fem" = gen_fem3d_device(110, 110, 110, 3) (3.99 M rows, 318 M non-zeros),
"powerlaw" = gen_powerlaw_device(1 M, 1 M, 6, 1.2, 400 000), "small" = a 200 k-row config-4 for trying the tool out: the matrices of
tools/edge_op_bench.py.
The 64-bit row and column indices of "gather" are built once, outside every timed region.  Per (H, d): the forward alone (no autograd
graph) and forward + backward (the gradients of x_dst and x_src), each side timed between HIP events over --rounds rounds of `reps`
calls, the sides in ALTERNATING rounds after one untimed warm-up step per side (engine, A^T and tables are built there); reps is chosen
per record so that a round of the slowest side lasts about --round-ms.  Per baseline: "ratio" = baseline median / edge_dot median (> 1:
edge_dot is faster), "spread" = (max - min) / median of a side's rounds, "verdict": "edge_dot" / the baseline's name when that side's
slowest round beats the other's fastest -- a difference larger than the spread between repeats -- else "undecided" (DESIGN 4.12).
"peak_bytes": torch.cuda.max_memory_allocated over one forward + backward step of a side (forward only for "weight_rows"), above what
was allocated before it (the operands, the upstream gradient and the matrix are allocated before it on every side).  A side that cannot
be allocated is recorded as such ("out of memory") and the others are timed without it; operands that cannot be allocated end the
record.  "bytes_per_entry": what each forward must at least move per stored entry -- edge_dot: the 4-byte column index, a gathered
x_src row and the scores (4 + 4 H d + 4 H; the x_dst row is read once per row at best); sddmm_loop: the column index once per head and
the stack's read and write (4 H + 4 H d + 12 H); gather: two 8-byte indices, each gather's read and write, the product's two reads and
one write, the sum's read and write (16 + 28 H d + 4 H).
--tag NAME is written into every record and says which build it timed."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASELINES = ("sddmm_loop", "gather", "weight_rows")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", choices=["config4", "fem", "powerlaw", "small"], default="small")
    ap.add_argument("--heads", default="1,8")
    ap.add_argument("--dims", default="16,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-ms", type=float, default=200.0)
    ap.add_argument("--max-reps", type=int, default=8)
    ap.add_argument("--tag", default="", help="written into every record as \"tag\" (names the build that was timed)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from sextans_amd import api, torch_op
    from sextans_amd._op_cache import _pattern_entry_of
    from sextans_amd.edge_dot import edge_dot
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

    def compare(name, f, c):
        r = stats(c)
        r["ratio"] = r["median_us"] / statistics.median(f)
        r["verdict"] = "edge_dot" if max(f) < min(c) else name if max(c) < min(f) else "undecided"
        return r

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    def uniform(*shape):
        return torch.rand(shape, device=dev, generator=gen).mul_(2.0).sub_(1.0)

    for H in [int(x) for x in args.heads.split(",") if x]:
        for d in [int(x) for x in args.dims.split(",") if x]:
            xd = xs = G = W = None
            try:
                xd, xs = uniform(M, H, d).requires_grad_(), uniform(K, H, d).requires_grad_()
                G = uniform(nnz, H)
                W = torch.zeros((nnz, H), device=dev)   # weight_rows' output (and the S its row pass loads without using it)
            except torch.OutOfMemoryError:
                del xd, xs, G, W
                torch.cuda.empty_cache()
                emit({"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "H": H, "d": d, "operands": "out of memory",
                      "operand_bytes": 4 * (H * d * (K + M) + 2 * nnz * H)})
                continue
            leaves = [xd, xs]

            def weight_rows():
                ent, stream, _, _, _ = _pattern_entry_of(A, False)
                ent.eng.score_attention_backward_device(api.SCORE_WEIGHT, H, d, W.data_ptr(), H, xs.data_ptr(), H * d, None, H * d, None,
                                                        xd.data_ptr(), H * d, W.data_ptr(), H, None, H * d, None, stream)
                return W

            def apply(side):
                if side == "edge_dot":
                    return edge_dot(A, xd, xs)
                if side == "sddmm_loop":
                    return torch.stack([torch_op.sddmm(A, xd[:, h], xs[:, h]).values() for h in range(H)], dim=1)
                if side == "gather":
                    return (xd[rows64] * xs[col64]).sum(-1)
                return weight_rows()

            def forward(side):
                with torch.no_grad():
                    apply(side)

            def step(side):
                for x in leaves:
                    x.grad = None
                if side == "weight_rows":   # (no backward of its own: forward only, everywhere)
                    return forward(side)
                apply(side).backward(G)

            torch_op.clear_cache()
            rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "H": H, "d": d, "rounds": args.rounds,
                   "bytes_per_entry": {"edge_dot_forward_at_least": 4 + 4 * H * d + 4 * H, "sddmm_loop_forward_at_least": 4 * H + 4 * H * d + 12 * H,
                                       "gather_forward_at_least": 16 + 28 * H * d + 4 * H}}
            if args.tag:
                rec["tag"] = args.tag
            sides = ["edge_dot"] + list(BASELINES)
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
                if "edge_dot" not in sides:   # (a training step does not fit next to the operands: nothing to compare)
                    break
            rec["peak_bytes"] = peak
            if "edge_dot" not in sides:
                emit(rec)
                torch_op.clear_cache()
                del xd, xs, G, W, leaves
                torch.cuda.empty_cache()
                continue
            rec["value_refreshes_after_warmup"] = torch_op.cache_info()["value_refreshes"]   # (sddmm_loop's backward refreshes; edge_dot never)
            for name, fn in (("forward", forward), ("forward_backward", step)):
                run = [s for s in sides if not (name == "forward_backward" and s == "weight_rows")]
                once = {}
                for s in list(run):
                    try:
                        once[s] = timed(lambda: fn(s), 1)
                    except torch.OutOfMemoryError:   # (the step fitted once, or the other way round)
                        torch.cuda.empty_cache()
                        run.remove(s)
                        rec[s] = "out of memory"
                reps = int(max(1, min(args.max_reps, args.round_ms * 1e3 / max(once.values()))))
                ts = {s: [] for s in run}
                for _ in range(args.rounds):   # alternating rounds
                    for s in ts:
                        ts[s].append(timed(lambda: fn(s), reps))
                rec[name] = {"edge_dot": stats(ts["edge_dot"]), "reps": reps}
                for s in run[1:]:
                    rec[name][s] = compare(s, ts["edge_dot"], ts[s])
                for x in leaves:
                    x.grad = None
                torch.cuda.empty_cache()
            emit(rec)
            torch_op.clear_cache()
            del xd, xs, G, W, leaves
            torch.cuda.empty_cache()
    if args.out:   # per workload: does edge_dot beat each baseline by more than the spread between repeats?
        with open(args.out) as fh:
            recs = [r for r in map(json.loads, fh) if r["matrix"] == args.matrix and "forward" in r]
        for name in ("forward", "forward_backward"):
            for b in BASELINES:
                verdicts = ["H%d d%d %s" % (r["H"], r["d"], "%s x%.2f" % (r[name][b]["verdict"], r[name][b]["ratio"]) if b in r[name]
                                            else r.get(b, "not run")) for r in recs]
                if name == "forward" or b != "weight_rows":
                    print("%s %s vs %s: %s" % (args.matrix, name, b, "; ".join(verdicts)))


if __name__ == "__main__":
    main()
