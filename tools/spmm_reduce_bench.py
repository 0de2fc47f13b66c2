"""spmm_reduce(A, B, "amax") against the composition torch allows on a GPU -- materialise the (nnz, N) products val[:, None] * B[col],
then scatter_reduce(..., "amax", include_self=False) over the row index (or torch.segment_reduce over the row lengths), autograd
through it -- on the same commit, the same process and the same tensors, on one GPU.

    python tools/spmm_reduce_bench.py --matrix config4 --out profiles/spmm_reduce.jsonl     (appends one record per N)
    python tools/spmm_reduce_bench.py --matrix small --dims 16,64

Matrices, rounds, "ratio", "spread", "verdict", "peak_bytes" and --tag: tools/compare_bench.py.
The composition's nnz-long row-index vector (and the row lengths) are built once, outside every timed region.  Per N: the forward alone
and forward + backward (the gradient of B; --grad-a: of A's values too).
A composition case that cannot be allocated is recorded as such ("composition": "out of memory") and the fused side is timed alone.
"spmm_sum": torch_op.spmm (the strict sum product) on the same matrix and N, for information: it does the same gathers.
"torch_sparse_mm_gpu": what torch.sparse.mm(A, B, "amax") of the installed GPU build does on a 1000-row corner of the matrix.
--fused-only times spmm_reduce alone (kernel tuning between two builds): no composition, no verdict."""
import argparse

import compare_bench as cb


def main():
    ap = argparse.ArgumentParser()
    cb.add_protocol_args(ap)
    ap.add_argument("--dims", default="16,64")
    ap.add_argument("--reduce", choices=["amax", "amin"], default="amax")
    ap.add_argument("--composition", choices=["scatter", "segment"], default="scatter", help="scatter_reduce over the row index, or segment_reduce")
    ap.add_argument("--grad-a", action="store_true", help="forward + backward also takes the gradient of A's values")
    ap.add_argument("--fused-only", action="store_true", help="time spmm_reduce alone (kernel tuning): no composition, no verdict")
    args = ap.parse_args()
    import torch
    from sextans_amd import torch_op
    dev = torch.device("cuda", 0)
    A, crow, col, val, M, K, nnz = cb.load_matrix(args.matrix)
    vleaf = val.detach().clone()               # the composition's values: a dense leaf
    if args.grad_a:
        A.requires_grad_(); vleaf.requires_grad_()
    gen = torch.Generator(device=dev).manual_seed(1)
    lens = (crow[1:] - crow[:-1]).long()
    row = torch.repeat_interleave(torch.arange(M, device=dev), lens, output_size=nnz)   # built once, untimed
    col64 = col.long()
    red = args.reduce

    try:   # what the installed torch does with the sparse op itself on this device
        rows = min(M, 1000)
        n0 = int(crow[rows].item())
        A0 = torch.sparse_csr_tensor(crow[:rows + 1].clone(), col[:n0].clone(), val[:n0].clone(), size=(rows, K))
        torch.sparse.mm(A0, torch.zeros((K, 8), device=dev), red)
        torch.cuda.synchronize()
        sparse_mm = "ok"
    except Exception as e:   # noqa: BLE001 (the message is the record)
        sparse_mm = "%s: %s" % (type(e).__name__, str(e).split("\n")[0][:200])

    def composition(B):
        P = vleaf[:, None] * B[col64]          # (nnz, N), materialised
        if args.composition == "segment":
            return torch.segment_reduce(P, "max" if red == "amax" else "min", lengths=lens, axis=0)
        out = torch.zeros((M, B.shape[1]), dtype=P.dtype, device=dev)
        return out.scatter_reduce(0, row[:, None].expand(-1, B.shape[1]), P, red, include_self=False)

    for N in [int(t) for t in args.dims.split(",") if t]:
        B = (torch.rand((K, N), device=dev, generator=gen) * 2 - 1).requires_grad_()
        G = torch.rand((M, N), device=dev, generator=gen) * 2 - 1
        leaves = (B, A, vleaf) if args.grad_a else (B,)

        def apply(side):
            if side == "fused":
                return torch_op.spmm_reduce(A, B, red)
            if side == "sum":
                return torch_op.spmm(A, B)
            return composition(B)

        def forward(side):
            with torch.no_grad():
                apply(side)

        def step(side):
            for t in leaves:
                t.grad = None
            apply(side).backward(G)

        torch_op.clear_cache()
        rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "reduce": red, "rounds": args.rounds,
               "composition_form": args.composition + "_reduce", "grad_a": bool(args.grad_a), "torch_sparse_mm_gpu": sparse_mm}
        if args.tag:
            rec["tag"] = args.tag
        sides = ["fused"] if args.fused_only else ["fused", "composition"]
        peak = {}
        for side, nbytes in cb.warm_up_peaks(step, leaves, sides + ["sum"], may_fail=["composition"]):
            if nbytes is None:
                sides.remove("composition")
                rec["composition"] = "out of memory"
            else:
                peak[side] = nbytes
        rec["peak_bytes"] = peak
        rec["value_refreshes"] = torch_op.cache_info()["value_refreshes"]
        for name, fn in (("forward", forward), ("forward_backward", step)):
            ts, reps = cb.alternating_rounds(fn, sides, args, also=["sum"])
            rec[name] = cb.pass_block(ts)
            rec[name]["spmm_sum"] = cb.stats(ts["sum"])
            rec[name]["reps"] = reps
        cb.emit(rec, args.out)
        torch_op.clear_cache()
        del B, G, leaves
        torch.cuda.empty_cache()
    if args.out and not args.fused_only:
        recs = cb.read_records(args.out, args.matrix)
        for name in cb.PASSES:
            cb.summary_line(recs, args.matrix, name, lambda r: "N%d" % r["N"], lambda r: r[name])


if __name__ == "__main__":
    main()
