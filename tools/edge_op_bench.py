"""edge_op.edge_op(A, x_dst, x_src, E, op) against the composition torch allows on a GPU -- x_dst[rows] (op) x_src[cols] (+ E) with the
gathers by torch_op.entry_rows(A) and A.col_indices() as 64-bit indices, autograd through index_add_ (float atomics) -- in the same
process on the same tensors, on one GPU.  The composition calls nothing of this library inside its timed region, so it is what the parent
commit offers.

    python tools/edge_op_bench.py --matrix config4 --out profiles/edge_op.jsonl     (appends one record per N and case)
    python tools/edge_op_bench.py --matrix small --dims 16,64 --cases add,add_e,mul

Matrices, rounds, "ratio", "spread", "verdict", "peak_bytes" and --tag: tools/compare_bench.py.
Cases: "add" (no E), "add_e" (with E), "mul" (no E).
The composition's 64-bit row and column indices are built once, outside every timed region.  Per N and case: the forward alone and
forward + backward (the gradients of x_dst, x_src and -- "add_e" -- E); the operands, the upstream gradient and the matrix are allocated
before a side's peak is taken.  A composition case that cannot be allocated is recorded as such ("composition": "out of memory") and the
fused side is timed alone; operands that cannot be allocated end the record.
"bytes_per_entry": what each forward must at least move per stored entry -- fused: the 4-byte column index, a gathered x_src row and
the Z row (4 + 8 N; + 4 N with E; the x_dst row is read once per row); composition: two 8-byte indices, each gather's read and write,
the elementwise pass's two reads and one write (16 + 28 N; + 12 N with E)."""
import argparse

import compare_bench as cb

CASES = {"add": ("add", False), "add_e": ("add", True), "mul": ("mul", False)}


def main():
    ap = argparse.ArgumentParser()
    cb.add_protocol_args(ap)
    ap.add_argument("--dims", default="16,64")
    ap.add_argument("--cases", default="add,add_e,mul")
    args = ap.parse_args()
    import torch
    from sextans_amd import torch_op
    from sextans_amd.edge_op import edge_op
    dev = torch.device("cuda", 0)
    A, crow, col, val, M, K, nnz = cb.load_matrix(args.matrix)
    gen = torch.Generator(device=dev).manual_seed(1)
    rows64 = torch_op.entry_rows(A)            # built once, untimed
    col64 = col.long()

    def composition(op, xd, xs, E):
        d, s = xd[rows64], xs[col64]           # two (nnz, N) gathers, materialised
        z = d + s if op == "add" else d * s
        return z + E if E is not None else z

    def uniform(rows, N):
        return torch.rand((rows, N), device=dev, generator=gen).mul_(2.0).sub_(1.0)

    for N in [int(x) for x in args.dims.split(",") if x]:
        for case in [x for x in args.cases.split(",") if x]:
            op, with_e = CASES[case]
            xd = xs = E = G = None
            try:
                xd, xs = uniform(M, N).requires_grad_(), uniform(K, N).requires_grad_()
                G = uniform(nnz, N)
                E = uniform(nnz, N).requires_grad_() if with_e else None
            except torch.OutOfMemoryError:
                del xd, xs, E, G
                torch.cuda.empty_cache()
                cb.emit({"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "case": case, "operands": "out of memory",
                         "operand_bytes": 4 * N * (K + M + nnz * (2 if with_e else 1))}, args.out)
                continue
            leaves = [x for x in (xd, xs, E) if x is not None]

            def apply(side):
                return edge_op(A, xd, xs, E, op=op) if side == "fused" else composition(op, xd, xs, E)

            def forward(side):
                with torch.no_grad():
                    apply(side)

            def step(side):
                for x in leaves:
                    x.grad = None
                apply(side).backward(G)

            torch_op.clear_cache()
            rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "case": case, "rounds": args.rounds,
                   "composition_form": "x_dst[entry_rows] op x_src[col_indices] (+ E), int64 indices, autograd through index_add_",
                   "grads": ", ".join(("x_dst", "x_src", "E") if with_e else ("x_dst", "x_src")),
                   "bytes_per_entry": {"fused_forward_at_least": 4 + (12 if with_e else 8) * N,
                                       "composition_forward_at_least": 16 + (40 if with_e else 28) * N}}
            if args.tag:
                rec["tag"] = args.tag
            sides = ["fused", "composition"]
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
                if "fused" not in sides:   # (a training step does not fit next to the operands: nothing to compare)
                    break
            rec["peak_bytes"] = peak
            if "fused" not in sides:
                cb.emit(rec, args.out)
                torch_op.clear_cache()
                del xd, xs, E, G, leaves
                torch.cuda.empty_cache()
                continue
            rec["value_refreshes"] = torch_op.cache_info()["value_refreshes"]
            for name, fn in (("forward", forward), ("forward_backward", step)):
                once, lost = cb.slowest_once_dropping(fn, sides)
                if lost:
                    rec["composition"] = "out of memory"
                ts, reps = cb.rounds_at(fn, sides, once, args)
                rec[name] = cb.pass_block(ts)
                rec[name]["reps"] = reps
                for x in leaves:
                    x.grad = None
                torch.cuda.empty_cache()
            cb.emit(rec, args.out)
            torch_op.clear_cache()
            del xd, xs, E, G, leaves
            torch.cuda.empty_cache()
    if args.out:
        recs = [r for r in cb.read_records(args.out, args.matrix) if "forward" in r]
        for name in cb.PASSES:
            cb.summary_line(recs, args.matrix, name, lambda r: "N%d %s" % (r["N"], r["case"]), lambda r: r[name])


if __name__ == "__main__":
    main()
