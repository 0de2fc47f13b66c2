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

Matrices, rounds, "ratio", "spread", "verdict", "peak_bytes" and --tag: tools/compare_bench.py; ratio and verdict stand per baseline, on
the baseline's block, with "edge_dot" / the baseline's name as the verdict's words.
The 64-bit row and column indices of "gather" are built once, outside every timed region.  Per (H, d): the forward alone and forward +
backward (the gradients of x_dst and x_src); "peak_bytes" is of the forward only for "weight_rows" (the operands, the upstream gradient
and the matrix are allocated before it on every side).  A side that cannot be allocated is recorded as such ("out of memory") and the
others are timed without it; operands that cannot be allocated end the record.  "bytes_per_entry": what each forward must at least move per stored entry -- edge_dot: the 4-byte column index, a gathered
x_src row and the scores (4 + 4 H d + 4 H; the x_dst row is read once per row at best); sddmm_loop: the column index once per head and
the stack's read and write (4 H + 4 H d + 12 H); gather: two 8-byte indices, each gather's read and write, the product's two reads and
one write, the sum's read and write (16 + 28 H d + 4 H)."""
import argparse

import compare_bench as cb

BASELINES = ("sddmm_loop", "gather", "weight_rows")


def main():
    ap = argparse.ArgumentParser()
    cb.add_protocol_args(ap)
    ap.add_argument("--heads", default="1,8")
    ap.add_argument("--dims", default="16,64")
    args = ap.parse_args()
    import torch
    from sextans_amd import api, torch_op
    from sextans_amd._op_cache import _pattern_entry_of
    from sextans_amd.edge_dot import edge_dot
    dev = torch.device("cuda", 0)
    A, crow, col, val, M, K, nnz = cb.load_matrix(args.matrix)
    gen = torch.Generator(device=dev).manual_seed(1)
    rows64 = torch_op.entry_rows(A)            # built once, untimed
    col64 = col.long()

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
                cb.emit({"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "H": H, "d": d, "operands": "out of memory",
                         "operand_bytes": 4 * (H * d * (K + M) + 2 * nnz * H)}, args.out)
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
            for side, nbytes in cb.warm_up_peaks(step, leaves, tuple(sides), may_fail=tuple(sides)):
                if nbytes is None:
                    sides.remove(side)
                    rec[side] = "out of memory"
                else:
                    peak[side] = nbytes
                for x in leaves:
                    x.grad = None
                torch.cuda.empty_cache()
                if "edge_dot" not in sides:   # (a training step does not fit next to the operands: nothing to compare)
                    break
            rec["peak_bytes"] = peak
            if "edge_dot" not in sides:
                cb.emit(rec, args.out)
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
                        once[s] = cb.timed(lambda: fn(s), 1)
                    except torch.OutOfMemoryError:   # (the step fitted once, or the other way round)
                        torch.cuda.empty_cache()
                        run.remove(s)
                        rec[s] = "out of memory"
                ts, reps = cb.rounds_at(fn, run, max(once.values()), args)
                rec[name] = {"edge_dot": cb.stats(ts["edge_dot"]), "reps": reps}
                for s in run[1:]:
                    rec[name][s] = cb.baseline_block(ts["edge_dot"], ts[s], "edge_dot", s)
                for x in leaves:
                    x.grad = None
                torch.cuda.empty_cache()
            cb.emit(rec, args.out)
            torch_op.clear_cache()
            del xd, xs, G, W, leaves
            torch.cuda.empty_cache()
    if args.out:
        recs = [r for r in cb.read_records(args.out, args.matrix) if "forward" in r]
        for name in cb.PASSES:
            for b in BASELINES:
                if name == "forward" or b != "weight_rows":
                    cb.summary_line(recs, args.matrix, "%s vs %s" % (name, b), lambda r: "H%d d%d" % (r["H"], r["d"]), lambda r: r[name].get(b),
                                    lambda r: r.get(b, "not run"))


if __name__ == "__main__":
    main()
