"""The price of attention dropout inside the fused kernels: the fused dropout entry (p = 0.6) against the SAME fused entry without dropout,
on the same commit, the same process and the same tensors, on one GPU.  What is timed is the hash: two 64-bit multiplies per
(entry, head), repeated in the T lanes of a slot.

    python tools/attention_dropout_bench.py --matrix config4 --family gat,gatv2 --out profiles/attention_dropout.jsonl
    python tools/attention_dropout_bench.py --matrix small --family attention --heads 1 --dims 16

Matrices as in tools/gat_attention_bench.py: "config4" = gen_csr_device(4 M, 4 M, Poisson(40)), "fem" = gen_fem3d_device(110, 110, 110, 3),
"powerlaw" = gen_powerlaw_device(1 M, 1 M, 6, 1.2, 400 000), "small" = a 200 k-row config-4 for trying the tool out.
Families: "gat" (gat_attention_dropout), "gatv2" (gatv2_attention_dropout), "attention" (sparse_attention_dropout(fused=True)).  Per
(family, H, d): the forward alone (no autograd graph) and forward + backward, each side timed between HIP events over --rounds rounds of
`reps` calls, the two sides in ALTERNATING rounds after one untimed warm-up step per side; reps is chosen per record so that a round
lasts about --round-ms.  "ratio" = dropout median / plain median (> 1: the hash costs time), "spread" = (max - min) / median of a
side's rounds, "verdict": "costs" when the dropout side's fastest round is slower than the plain side's slowest -- a difference larger
than the spread between repeats --, "faster" the other way round, else "within_spread".
For "attention" a second comparison, "vs_composition": the fused dropout entry against sparse_attention_dropout(fused=False), which
materialises S, P and the mask per head; ratio = composition median / fused median, and "peak_bytes" of one forward + backward step of
each (torch.cuda.max_memory_allocated above what was allocated before it).  --no-composition leaves it out (it needs tens of GB on the
large matrices)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P_DROP, SEED = 0.6, 2024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", choices=["config4", "fem", "powerlaw", "small"], default="small")
    ap.add_argument("--family", default="gat,gatv2")
    ap.add_argument("--heads", default="1,8")
    ap.add_argument("--dims", default="16,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-ms", type=float, default=200.0)
    ap.add_argument("--max-reps", type=int, default=8)
    ap.add_argument("--slope", type=float, default=0.2)
    ap.add_argument("--no-composition", action="store_true")
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

    def uniform(*shape):
        return (torch.rand(shape, device=dev, generator=gen) * 2 - 1) * 0.5

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

    def versus(fn, sides):
        """alternating rounds of the sides -> (their statistics, the rounds' times)"""
        once = max(timed(lambda: fn(s), 1) for s in sides)
        reps = int(max(1, min(args.max_reps, args.round_ms * 1e3 / once)))
        ts = {s: [] for s in sides}
        for _ in range(args.rounds):
            for s in sides:
                ts[s].append(timed(lambda: fn(s), reps))
        r = {s: stats(ts[s]) for s in sides}
        r["reps"] = reps
        return r, ts

    for fam in [t for t in args.family.split(",") if t]:
        for H in [int(t) for t in args.heads.split(",") if t]:
            for d in [int(t) for t in args.dims.split(",") if t]:
                if fam == "gat":
                    params = [uniform(M, H).requires_grad_(), uniform(K, H).requires_grad_(), uniform(K, H, d).requires_grad_()]
                elif fam == "gatv2":
                    params = [uniform(M, H, d).requires_grad_(), uniform(K, H, d).requires_grad_(), uniform(H, d).requires_grad_()]
                else:
                    params = [uniform(M, H, d).requires_grad_(), uniform(K, H, d).requires_grad_(), uniform(K, H, d).requires_grad_()]
                G = torch.rand((M, H, d), device=dev, generator=gen) * 2 - 1

                def apply(side):
                    drop = 0.0 if side == "plain" else P_DROP
                    if fam == "gat":
                        return torch_op.gat_attention_dropout(A, *params, drop, seed=SEED, negative_slope=args.slope)
                    if fam == "gatv2":
                        return torch_op.gatv2_attention_dropout(A, *params, drop, seed=SEED, negative_slope=args.slope)
                    return torch_op.sparse_attention_dropout(A, *params, drop, seed=SEED, fused=side != "composition")

                def forward(side):
                    with torch.no_grad():
                        apply(side)

                def step(side):
                    for t in params:
                        t.grad = None
                    apply(side).backward(G)

                torch_op.clear_cache()
                rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": int(nnz), "family": fam, "H": H, "d": d, "p": P_DROP, "rounds": args.rounds}
                for side in ("dropout", "plain"):   # warm-up: engine, A^T, tables
                    step(side)
                torch.cuda.synchronize()
                for name, fn in (("forward", forward), ("forward_backward", step)):
                    r, ts = versus(fn, ("plain", "dropout"))
                    r["ratio"] = r["dropout"]["median_us"] / r["plain"]["median_us"]
                    r["verdict"] = ("costs" if min(ts["dropout"]) > max(ts["plain"]) else
                                    "faster" if max(ts["dropout"]) < min(ts["plain"]) else "within_spread")
                    rec[name] = r
                if fam == "attention" and not args.no_composition:
                    comp = {"peak_bytes": {}}
                    for side in ("dropout", "composition"):
                        step(side)          # (warm-up of the composition: its plans)
                        for t in params:
                            t.grad = None
                        torch.cuda.synchronize()
                        torch.cuda.reset_peak_memory_stats(dev)
                        base = torch.cuda.memory_allocated(dev)
                        step(side)
                        torch.cuda.synchronize()
                        comp["peak_bytes"]["fused" if side == "dropout" else side] = int(torch.cuda.max_memory_allocated(dev) - base)
                    for name, fn in (("forward", forward), ("forward_backward", step)):
                        r, ts = versus(fn, ("dropout", "composition"))
                        r["ratio"] = r["composition"]["median_us"] / r["dropout"]["median_us"]
                        r["verdict"] = ("fused" if max(ts["dropout"]) < min(ts["composition"]) else
                                        "composition" if max(ts["composition"]) < min(ts["dropout"]) else "undecided")
                        comp[name] = r
                    rec["vs_composition"] = comp
                line = json.dumps(rec)
                print(line, flush=True)
                if args.out:
                    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                    with open(args.out, "a") as fh:
                        fh.write(line + "\n")
                torch_op.clear_cache()
                del params, G
    if args.out:
        with open(args.out) as fh:
            recs = [r for r in map(json.loads, fh) if r["matrix"] == args.matrix]
        for name in ("forward", "forward_backward"):
            print("%s %s: %s" % (args.matrix, name, "; ".join("%s H%d d%d %s x%.3f" % (r["family"], r["H"], r["d"], r[name]["verdict"],
                                                                                      r[name]["ratio"]) for r in recs)))


if __name__ == "__main__":
    main()
