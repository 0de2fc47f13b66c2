"""sextans_amd.gated.spmm_gated against the composition a user is left with without it -- z = x_dst[rows] + x_src[cols] (+ E), materialised
as (nnz, N) tensors, torch.sigmoid, torch_op.spmm_edge(A, V, g, "mul"), for the normalised mode torch_op.spmm_edge(A, None, g, "copy") and
a division, autograd through all of it (the gathers' backward is an atomic index_add_) -- on the same commit, the same process and the
same tensors, on one GPU.

    python tools/spmm_gated_bench.py --matrix config4 --out profiles/spmm_gated.jsonl     (appends one record per N, mode and E / no E)
    python tools/spmm_gated_bench.py --matrix small --dims 16,64

Matrices, rounds, "ratio", "spread", "verdict" and "peak_bytes": tools/compare_bench.py.
The composition's 64-bit row and column indices are built once, outside every timed region.  Per record: the forward alone and forward +
backward (the gradients of x_dst, x_src, V and, when present, E); the operands, E among them, are allocated before a side's peak is taken.
A case whose operands or whose composition cannot be allocated is recorded as such ("operands": "out of memory" / "composition": "out of
memory"); in the second case the fused side is timed alone."""
import argparse

import compare_bench as cb


def main():
    ap = argparse.ArgumentParser()
    cb.add_protocol_args(ap, tag=False)
    ap.add_argument("--dims", default="16,64")
    ap.add_argument("--modes", default="sum,norm")
    ap.add_argument("--edge", default="0,1", help="0: without E, 1: with E")
    args = ap.parse_args()
    import torch
    from sextans_amd import torch_op
    from sextans_amd.gated import spmm_gated
    dev = torch.device("cuda", 0)
    A, crow, col, val, M, K, nnz = cb.load_matrix(args.matrix)
    gen = torch.Generator(device=dev).manual_seed(1)
    lens = (crow[1:] - crow[:-1]).long()       # built once, untimed
    row64 = torch.repeat_interleave(torch.arange(M, device=dev), lens, output_size=nnz)
    col64 = col.long()
    eps = 1e-6

    def composition(xd, xs, V, E, norm):
        z = xd[row64] + xs[col64]              # (nnz, N), materialised
        if E is not None:
            z = z + E
        g = torch.sigmoid(z)
        num = torch_op.spmm_edge(A, V, g, "mul")
        if not norm:
            return num
        return num / (torch_op.spmm_edge(A, None, g, "copy") + eps)

    cases = [(int(n), m, e == "1") for n in args.dims.split(",") if n for m in args.modes.split(",") if m for e in args.edge.split(",") if e]
    for N, mode, with_e in cases:
        norm = mode == "norm"
        rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "mode": mode, "edge_features": with_e, "rounds": args.rounds,
               "composition_form": "gathers, sigmoid, spmm_edge mul" + (", spmm_edge copy, division" if norm else ""),
               "grads": "x_dst, x_src, V" + (", E" if with_e else "")}
        torch_op.clear_cache()
        try:
            rand = lambda rows: (torch.rand((rows, N), device=dev, generator=gen) * 2 - 1)   # noqa: E731
            xd, xs, V = rand(M).requires_grad_(), rand(K).requires_grad_(), rand(K).requires_grad_()
            E = rand(nnz).requires_grad_() if with_e else None
            G = rand(M)
        except torch.OutOfMemoryError:
            xd = xs = V = E = G = None
            torch.cuda.empty_cache()
            rec["operands"] = "out of memory"
            cb.emit(rec, args.out)
            continue
        leaves = [t for t in (xd, xs, V, E) if t is not None]

        def apply(side):
            if side == "fused":
                return spmm_gated(A, xd, xs, V, E, normalize=norm, eps=eps)
            return composition(xd, xs, V, E, norm)

        def forward(side):
            with torch.no_grad():
                apply(side)

        def step(side):
            for x in leaves:
                x.grad = None
            apply(side).backward(G)

        sides = ["fused", "composition"]
        peak = {}
        for side, nbytes in cb.warm_up_peaks(step, leaves, tuple(sides), may_fail=["composition"]):
            if nbytes is None:
                sides.remove("composition")
                rec["composition"] = "out of memory"
            else:
                peak[side] = nbytes
        rec["peak_bytes"] = peak
        rec["value_refreshes"] = torch_op.cache_info()["value_refreshes"]
        for name, fn in (("forward", forward), ("forward_backward", step)):
            for x in leaves:
                x.grad = None
            once, lost = cb.slowest_once_dropping(fn, sides)
            if lost:
                rec["composition"] = "out of memory"
            ts, reps = cb.rounds_at(fn, sides, once, args)
            rec[name] = cb.pass_block(ts)
            rec[name]["reps"] = reps
        cb.emit(rec, args.out)
        torch_op.clear_cache()
        del xd, xs, V, E, G, leaves
        torch.cuda.empty_cache()
    if args.out:
        recs = [r for r in cb.read_records(args.out, args.matrix) if "forward" in r]
        for name in cb.PASSES:
            cb.summary_line(recs, args.matrix, name, lambda r: "N%d %s%s" % (r["N"], r["mode"], "+E" if r["edge_features"] else ""), lambda r: r[name])


if __name__ == "__main__":
    main()
