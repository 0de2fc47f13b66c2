"""The price of attention dropout inside the fused kernels: the fused dropout entry (p = 0.6) against the SAME fused entry without dropout,
on the same commit, the same process and the same tensors, on one GPU.  What is timed is the hash: two 64-bit multiplies per
(entry, head), repeated in the T lanes of a slot.

    python tools/attention_dropout_bench.py --matrix config4 --family gat,gatv2 --out profiles/attention_dropout.jsonl
    python tools/attention_dropout_bench.py --matrix small --family attention --heads 1 --dims 16

Matrices, rounds, "spread" and "peak_bytes": tools/compare_bench.py.
Families: "gat" (gat_attention_dropout), "gatv2" (gatv2_attention_dropout), "attention" (sparse_attention_dropout(fused=True)).  Per
(family, H, d): the forward alone and forward + backward, plain and dropout in alternating rounds after one untimed warm-up step per side.
"ratio" = dropout median / plain median (> 1: the hash costs time); "verdict" is compare_bench's rule in this tool's words: "costs" when
the plain side wins (the dropout side's fastest round is slower than the plain side's slowest), "faster" when the dropout side wins, else
"within_spread".
For "attention" a second comparison, "vs_composition": the fused dropout entry against sparse_attention_dropout(fused=False), which
materialises S, P and the mask per head; ratio = composition median / fused median, verdict "fused" / "composition" / "undecided", and
"peak_bytes" of one forward + backward step of each.  --no-composition leaves it out (it needs tens of GB on the large matrices)."""
import argparse

import compare_bench as cb

P_DROP, SEED = 0.6, 2024
WORDS = {"plain": "costs", "dropout": "faster", "undecided": "within_spread"}


def main():
    ap = argparse.ArgumentParser()
    cb.add_protocol_args(ap, tag=False)
    ap.add_argument("--family", default="gat,gatv2")
    ap.add_argument("--heads", default="1,8")
    ap.add_argument("--dims", default="16,64")
    ap.add_argument("--slope", type=float, default=0.2)
    ap.add_argument("--no-composition", action="store_true")
    args = ap.parse_args()
    import torch
    from sextans_amd import torch_op
    dev = torch.device("cuda", 0)
    A, crow, col, val, M, K, nnz = cb.load_matrix(args.matrix)
    gen = torch.Generator(device=dev).manual_seed(1)

    def uniform(*shape):
        return (torch.rand(shape, device=dev, generator=gen) * 2 - 1) * 0.5

    def versus(fn, sides):
        """alternating rounds of the sides -> (their statistics, the rounds' times)"""
        ts, reps = cb.alternating_rounds(fn, sides, args)
        r = {s: cb.stats(ts[s]) for s in sides}
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
                rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "family": fam, "H": H, "d": d, "p": P_DROP, "rounds": args.rounds}
                for side in ("dropout", "plain"):   # warm-up: engine, A^T, tables
                    step(side)
                torch.cuda.synchronize()
                for name, fn in (("forward", forward), ("forward_backward", step)):
                    r, ts = versus(fn, ("plain", "dropout"))
                    r["ratio"], won = cb.verdict(ts["plain"], ts["dropout"], "plain", "dropout")
                    r["verdict"] = WORDS[won]
                    rec[name] = r
                if fam == "attention" and not args.no_composition:
                    peak = dict(cb.warm_up_peaks(step, params, ("dropout", "composition")))   # (warm-up of the composition: its plans)
                    comp = {"peak_bytes": {"fused": peak["dropout"], "composition": peak["composition"]}}
                    for name, fn in (("forward", forward), ("forward_backward", step)):
                        r, ts = versus(fn, ("dropout", "composition"))
                        r["ratio"], r["verdict"] = cb.verdict(ts["dropout"], ts["composition"])
                        comp[name] = r
                    rec["vs_composition"] = comp
                cb.emit(rec, args.out)
                torch_op.clear_cache()
                del params, G
    if args.out:
        recs = cb.read_records(args.out, args.matrix)
        for name in cb.PASSES:
            print("%s %s: %s" % (args.matrix, name, "; ".join("%s H%d d%d %s x%.3f" % (r["family"], r["H"], r["d"], r[name]["verdict"],
                                                                                      r[name]["ratio"]) for r in recs)))


if __name__ == "__main__":
    main()
