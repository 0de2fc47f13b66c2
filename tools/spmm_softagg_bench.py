"""spmm_softagg(A, B, t) against the composition torch allows on a GPU -- materialise the (nnz, N) products P = val[:, None] * B[col], then
torch.segment_reduce max of t P over the row lengths, exp, segment_reduce sum, the weighted segment_reduce sum, autograd through it -- on
the same commit, the same process and the same tensors, on one GPU.

    python tools/spmm_softagg_bench.py --matrix config4 --out profiles/spmm_softagg.jsonl     (appends one record per N)
    python tools/spmm_softagg_bench.py --matrix small --dims 16,64

Matrices, rounds, "ratio", "spread", "verdict", "peak_bytes" and --tag: tools/compare_bench.py.
The composition's row lengths and 64-bit column indices are built once, outside every timed region.  Per N: the forward alone and forward
+ backward (the gradients of B and of the (N,) temperature t).
A composition case that cannot be allocated is recorded as such ("composition": "out of memory") and the fused side is timed alone.
For information, on the same matrix and N: "spmm_reduce_amax" = one torch_op.spmm_reduce(A, B, "amax") pass (its backward: the gradient
of B), "spmm_sum" = torch_op.spmm, the strict sum product.  They do the same gathers.
--fused-only times spmm_softagg alone (kernel tuning between two builds): no composition, no verdict."""
import argparse

import compare_bench as cb


def main():
    ap = argparse.ArgumentParser()
    cb.add_protocol_args(ap)
    ap.add_argument("--dims", default="16,64")
    ap.add_argument("--fused-only", action="store_true", help="time spmm_softagg alone (kernel tuning): no composition, no verdict")
    args = ap.parse_args()
    import torch
    from sextans_amd import torch_op
    dev = torch.device("cuda", 0)
    A, crow, col, val, M, K, nnz = cb.load_matrix(args.matrix)
    vleaf = val.detach().clone()               # the composition's values
    gen = torch.Generator(device=dev).manual_seed(1)
    lens = (crow[1:] - crow[:-1]).long()       # built once, untimed
    col64 = col.long()

    def composition(B, t):
        P = vleaf[:, None] * B[col64]          # (nnz, N), materialised
        S = P * t
        m = torch.segment_reduce(S.detach(), "max", lengths=lens, axis=0)   # (only a reference point: no gradient through it)
        E = torch.exp(S - torch.repeat_interleave(m, lens, dim=0, output_size=nnz))
        z = torch.segment_reduce(E, "sum", lengths=lens, axis=0)
        acc = torch.segment_reduce(E * P, "sum", lengths=lens, axis=0)
        return acc / z.clamp(min=1e-30)

    extras = ["spmm_reduce_amax", "spmm_sum"]
    for N in [int(x) for x in args.dims.split(",") if x]:
        B = (torch.rand((K, N), device=dev, generator=gen) * 2 - 1).requires_grad_()
        t = (torch.rand((N,), device=dev, generator=gen) * 4 - 1).requires_grad_()   # temperatures in [-1, 3)
        G = torch.rand((M, N), device=dev, generator=gen) * 2 - 1
        leaves = (B, t)

        def apply(side):
            if side == "fused":
                return torch_op.spmm_softagg(A, B, t)
            if side == "spmm_reduce_amax":
                return torch_op.spmm_reduce(A, B, "amax")
            if side == "spmm_sum":
                return torch_op.spmm(A, B)
            return composition(B, t)

        def forward(side):
            with torch.no_grad():
                apply(side)

        def step(side):
            for x in leaves:
                x.grad = None
            apply(side).backward(G)

        torch_op.clear_cache()
        rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "rounds": args.rounds,
               "composition_form": "segment_reduce max, exp, sum, weighted sum", "grads": "B, t"}
        if args.tag:
            rec["tag"] = args.tag
        sides = ["fused"] if args.fused_only else ["fused", "composition"]
        peak = {}
        for side, nbytes in cb.warm_up_peaks(step, leaves, sides + extras, may_fail=["composition"]):
            if nbytes is None:
                sides.remove("composition")
                rec["composition"] = "out of memory"
            else:
                peak[side] = nbytes
        rec["peak_bytes"] = peak
        rec["value_refreshes"] = torch_op.cache_info()["value_refreshes"]
        for name, fn in (("forward", forward), ("forward_backward", step)):
            once, lost = cb.slowest_once_dropping(fn, sides)
            if lost:
                rec["composition"] = "out of memory"
            ts, reps = cb.rounds_at(fn, sides + extras, once, args)
            rec[name] = cb.pass_block(ts)
            for s in extras:
                rec[name][s] = cb.stats(ts[s])
            rec[name]["reps"] = reps
        cb.emit(rec, args.out)
        torch_op.clear_cache()
        del B, G, t, leaves
        torch.cuda.empty_cache()
    if args.out and not args.fused_only:
        recs = cb.read_records(args.out, args.matrix)
        for name in cb.PASSES:
            cb.summary_line(recs, args.matrix, name, lambda r: "N%d" % r["N"], lambda r: r[name])


if __name__ == "__main__":
    main()
