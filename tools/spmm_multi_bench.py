"""spmm_multi(A, B, aggr) against the composition of the project's own single-aggregation ops on the same commit, the same process and
the same tensors, on one GPU.  A has UNIT values, so that spmm(A, B * B) is the sum of squares of the messages: the composition is
spmm(A, B), spmm(A, B * B) (its (K, N) temporary B * B inside the timed region and the peak), spmm_reduce(A, B, "amax") and
spmm_reduce(A, B, "amin") -- those of them the aggregate set needs -- and the same elementwise mean / var / std formulas on top.

    python tools/spmm_multi_bench.py --matrix config4 --out profiles/spmm_multi.jsonl     (appends one record per N and aggregate set)
    python tools/spmm_multi_bench.py --matrix small --dims 16,64

Matrices, rounds, "ratio", "spread", "verdict", "peak_bytes" and --tag: tools/compare_bench.py.
Per N and aggregate set ("mean,max,min,std" and "mean,std"): the forward alone and forward + backward (the gradient of B).
"reduce_amax": one spmm_reduce(A, B, "amax") pass on the same matrix and N, for information: the fused
forward does the same gathers."""
import argparse

import compare_bench as cb


def main():
    ap = argparse.ArgumentParser()
    cb.add_protocol_args(ap)
    ap.add_argument("--dims", default="16,64")
    ap.add_argument("--aggr", default="mean,max,min,std;mean,std", help="aggregate sets, ';' between sets")
    args = ap.parse_args()
    import torch
    from sextans_amd import torch_op
    dev = torch.device("cuda", 0)
    crow, col, val, M, K, nnz = cb.load_matrix(args.matrix)[1:]
    A = torch.sparse_csr_tensor(crow, col, val.fill_(1.0), size=(M, K))   # unit values
    deg = (crow[1:] - crow[:-1]).clamp(min=1).to(torch.float32)[:, None]
    gen = torch.Generator(device=dev).manual_seed(1)
    eps = 1e-5

    def composition(B, aggr):
        raw = {}
        if any(x in aggr for x in ("sum", "mean", "var", "std")):
            raw["sum"] = torch_op.spmm(A, B)
        if any(x in aggr for x in ("sumsq", "var", "std")):
            raw["sumsq"] = torch_op.spmm(A, B * B)
        if "max" in aggr:
            raw["max"] = torch_op.spmm_reduce(A, B, "amax")
        if "min" in aggr:
            raw["min"] = torch_op.spmm_reduce(A, B, "amin")
        if "sum" in raw:
            raw["mean"] = raw["sum"] / deg
        if "sumsq" in raw:
            raw["var"] = raw["sumsq"] / deg - raw["mean"] ** 2
            raw["std"] = torch.sqrt(torch.relu(raw["var"]) + eps)
        return torch.cat([raw[x] for x in aggr], dim=1)

    for N in [int(t) for t in args.dims.split(",") if t]:
        for aggr in [tuple(s.split(",")) for s in args.aggr.split(";") if s]:
            B = (torch.rand((K, N), device=dev, generator=gen) * 2 - 1).requires_grad_()
            G = torch.rand((M, len(aggr) * N), device=dev, generator=gen) * 2 - 1

            def apply(side):
                if side == "fused":
                    return torch_op.spmm_multi(A, B, aggr, eps=eps)
                if side == "reduce_amax":
                    return torch_op.spmm_reduce(A, B, "amax")
                return composition(B, aggr)

            def forward(side):
                with torch.no_grad():
                    apply(side)

            def step(side):
                B.grad = None
                out = apply(side)
                out.backward(G if side != "reduce_amax" else G[:, :N])

            torch_op.clear_cache()
            rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "aggr": list(aggr), "rounds": args.rounds,
                   "composition_form": "spmm x2 + spmm_reduce x2, unit values"}
            if args.tag:
                rec["tag"] = args.tag
            sides = ["fused", "composition"]
            rec["peak_bytes"] = dict(cb.warm_up_peaks(step, (B,), sides + ["reduce_amax"]))
            rec["value_refreshes"] = torch_op.cache_info()["value_refreshes"]
            with torch.no_grad():   # the two sides compute the same thing
                diff = (apply("fused") - apply("composition")).abs().max().item()
            rec["max_abs_diff"] = diff
            for name, fn in (("forward", forward), ("forward_backward", step)):
                ts, reps = cb.alternating_rounds(fn, sides, args, also=["reduce_amax"])
                rec[name] = cb.two_sided(ts["fused"], ts["composition"])
                rec[name]["reduce_amax"] = cb.stats(ts["reduce_amax"])
                rec[name]["reps"] = reps
            cb.emit(rec, args.out)
            torch_op.clear_cache()
            del B, G
            torch.cuda.empty_cache()
    if args.out:
        recs = cb.read_records(args.out, args.matrix)
        for name in cb.PASSES:
            cb.summary_line(recs, args.matrix, name, lambda r: "N%d %s" % (r["N"], "+".join(r["aggr"])), lambda r: r[name])


if __name__ == "__main__":
    main()
