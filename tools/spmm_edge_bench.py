"""spmm_edge(A, B, E, "mul") against the compositions torch allows on a GPU -- gather B[col], multiply with E into a second (nnz, N)
tensor, then reduce it over the rows with torch.segment_reduce (over the row lengths) or with index_add_ (over the row index: float
atomics), autograd through it -- on the same commit, the same process and the same tensors, on one GPU.

    python tools/spmm_edge_bench.py --matrix config4 --out profiles/spmm_edge.jsonl     (appends one record per N)
    python tools/spmm_edge_bench.py --matrix small --dims 16,64

Matrices, rounds, "ratio", "spread", "verdict", "peak_bytes" and --tag: tools/compare_bench.py.
The compositions' nnz-long row-index vector (and the row lengths) are built once, outside every timed region.  Per N: the forward alone
and forward + backward (the gradients of B and E).  Per composition form ("segment_reduce", "index_add"), on the form's own block:
"ratio" = its median / the fused median, "verdict" "fused" / "composition" / "undecided".  B, E, G and the matrix are allocated before a
side's peak is taken.  A composition that cannot be allocated is recorded as "out of memory" and the other sides are timed without it.
"bytes_per_entry": the traffic the byte count of DESIGN 4.15 expects of the fused forward (4 + 8 N) and at least of the composition
(4 + 16 N), for reading the times against."""
import argparse

import compare_bench as cb

FORMS = ("segment_reduce", "index_add")


def main():
    ap = argparse.ArgumentParser()
    cb.add_protocol_args(ap)
    ap.add_argument("--dims", default="16,64")
    args = ap.parse_args()
    import torch
    from sextans_amd import torch_op
    dev = torch.device("cuda", 0)
    A, crow, col, val, M, K, nnz = cb.load_matrix(args.matrix)
    gen = torch.Generator(device=dev).manual_seed(1)
    lens = (crow[1:] - crow[:-1]).long()
    row = torch.repeat_interleave(torch.arange(M, device=dev), lens, output_size=nnz)   # built once, untimed
    col64 = col.long()

    for N in [int(t) for t in args.dims.split(",") if t]:
        B = (torch.rand((K, N), device=dev, generator=gen) * 2 - 1).requires_grad_()
        E = torch.rand((nnz, N), device=dev, generator=gen).mul_(2).sub_(1).requires_grad_()
        G = torch.rand((M, N), device=dev, generator=gen) * 2 - 1
        leaves = (B, E)

        def apply(side):
            if side == "fused":
                return torch_op.spmm_edge(A, B, E, "mul")
            P = B[col64] * E                       # two (nnz, N) tensors, materialised
            if side == "segment_reduce":
                return torch.segment_reduce(P, "sum", lengths=lens, axis=0)
            return torch.zeros((M, N), dtype=P.dtype, device=dev).index_add_(0, row, P)

        def forward(side):
            with torch.no_grad():
                apply(side)

        def step(side):
            for t in leaves:
                t.grad = None
            apply(side).backward(G)

        torch_op.clear_cache()
        rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "op": "mul", "rounds": args.rounds,
               "bytes_per_entry": {"fused_forward": 4 + 8 * N, "composition_forward_at_least": 4 + 16 * N}}
        if args.tag:
            rec["tag"] = args.tag
        sides = ["fused"] + list(FORMS)
        peak = {}
        for side in list(sides):   # warm-up, and the peak of one step
            try:
                peak[side] = cb.peak_of_step(lambda: step(side), leaves)
            except RuntimeError as e:   # (torch.OutOfMemoryError is one)
                if side == "fused":
                    raise
                sides.remove(side)
                rec[side] = "out of memory" if isinstance(e, torch.OutOfMemoryError) else "%s: %s" % (type(e).__name__, str(e).split("\n")[0][:200])
            for t in leaves:
                t.grad = None
            torch.cuda.empty_cache()
        rec["peak_bytes"] = peak
        rec["value_refreshes"] = torch_op.cache_info()["value_refreshes"]
        for name, fn in (("forward", forward), ("forward_backward", step)):
            ts, reps = cb.alternating_rounds(fn, sides, args)
            rec[name] = {"fused": cb.stats(ts["fused"]), "reps": reps}
            for s in sides[1:]:
                rec[name][s] = cb.baseline_block(ts["fused"], ts[s])
        cb.emit(rec, args.out)
        torch_op.clear_cache()
        del B, E, G, leaves
        torch.cuda.empty_cache()
    if args.out:
        recs = cb.read_records(args.out, args.matrix)
        for name in cb.PASSES:
            for form in FORMS:
                cb.summary_line(recs, args.matrix, "%s vs %s" % (name, form), lambda r: "N%d" % r["N"], lambda r: r[name].get(form),
                                lambda r: r.get(form, "not run"))


if __name__ == "__main__":
    main()
