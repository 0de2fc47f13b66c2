"""spmm_edge_multi(A, B, E, op, aggr) against the composition available on the same commit, in the same process and on the same tensors,
on one GPU: the messages materialised by torch (m = E for "copy", B[col] * E for "mul"), spmm_edge(A, None, m, "copy") for the sum,
spmm_edge(A, None, m * m, "copy") for the sum of squares, torch.segment_reduce(m, "max" / "min", offsets=crow) for the extrema -- those of
them the aggregate set needs --, the same elementwise mean / var / std formulas on top, and autograd through all of it.

    python tools/spmm_edge_multi_bench.py --matrix config4 --out profiles/spmm_edge_multi.jsonl   (appends one record per N, op and set)
    python tools/spmm_edge_multi_bench.py --matrix small --dims 16,64

Matrices, rounds, "ratio", "spread", "verdict", "peak_bytes" and --tag: tools/compare_bench.py.
Per N, op ("copy", "mul") and aggregate set ("mean,max,min,std" and "max"): the forward alone and forward + backward (the gradients of E
and, for "mul", of B); E and B are allocated before a side's peak is taken.  A side that cannot be allocated is recorded as
{"error": "out of memory"} and the record carries no verdict.  "max_abs_diff": fused against composition over the rows that hold an
entry (torch.segment_reduce gives an empty row -inf / +inf, the fused op 0)."""
import argparse

import compare_bench as cb


def main():
    ap = argparse.ArgumentParser()
    cb.add_protocol_args(ap)
    ap.add_argument("--dims", default="16,64")
    ap.add_argument("--ops", default="copy,mul")
    ap.add_argument("--aggr", default="mean,max,min,std;max", help="aggregate sets, ';' between sets")
    args = ap.parse_args()
    import torch
    from sextans_amd import torch_op
    dev = torch.device("cuda", 0)
    crow, col, val, M, K, nnz = cb.load_matrix(args.matrix)[1:]
    A = torch.sparse_csr_tensor(crow, col, val.fill_(1.0), size=(M, K))   # (only the pattern is used)
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

    for N in [int(t) for t in args.dims.split(",") if t]:
        for op in [t for t in args.ops.split(",") if t]:
            for aggr in [tuple(s.split(",")) for s in args.aggr.split(";") if s]:
                rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "op": op, "aggr": list(aggr), "rounds": args.rounds,
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
                    cb.emit(rec, args.out)
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

                leaves = [x for x in (E, B) if x is not None]

                def step(side):
                    for x in leaves:
                        x.grad = None
                    apply(side).backward(G)

                sides = ["fused", "composition"]
                peak, failed = {}, set()
                for side, nbytes in cb.warm_up_peaks(step, leaves, sides, may_fail=sides):
                    if nbytes is None:
                        failed.add(side)
                        peak[side] = {"error": "out of memory"}
                    else:
                        peak[side] = nbytes
                    for x in leaves:
                        x.grad = None
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
                    ts, reps = cb.alternating_rounds(fn, live, args)
                    rec[name] = cb.two_sided(ts["fused"], ts["composition"]) if len(live) == 2 else {live[0]: cb.stats(ts[live[0]])}
                    rec[name]["reps"] = reps
                cb.emit(rec, args.out)
                torch_op.clear_cache()
                del B, E, G, leaves
                torch.cuda.empty_cache()
    if args.out:
        recs = cb.read_records(args.out, args.matrix)
        for name in cb.PASSES:
            cb.summary_line(recs, args.matrix, name, lambda r: "N%d %s %s" % (r["N"], r["op"], "+".join(r["aggr"])), lambda r: r.get(name),
                            "not allocated")


if __name__ == "__main__":
    main()
