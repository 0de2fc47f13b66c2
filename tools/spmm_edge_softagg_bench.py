"""edge_softagg.spmm_edge_softagg(A, B, E, op, t) against the composition torch allows on a GPU -- materialise the (nnz, N) messages
(relu(B[col] + E) for "add_relu", GENConv's; E itself for "copy"), then torch.segment_reduce max of t m over the row lengths, exp,
segment_reduce sum, the weighted segment_reduce sum, autograd through it -- on the same commit, the same process and the same tensors,
on one GPU.

    python tools/spmm_edge_softagg_bench.py --matrix config4 --out profiles/spmm_edge_softagg.jsonl     (appends one record per N and op)
    python tools/spmm_edge_softagg_bench.py --matrix small --dims 16,64 --ops add_relu,copy

Matrices, rounds, "ratio", "spread", "verdict", "peak_bytes" and --tag: tools/compare_bench.py.
The composition's row lengths and 64-bit column indices are built once, outside every timed region.  Per N and op: the forward alone and
forward + backward (the gradients of B -- not for "copy" --, of E and of the (N,) temperature t); B, E, G, t and the matrix are allocated
before a side's peak is taken.  A composition case that cannot be allocated is recorded as such ("composition": "out of memory") and the
fused side is timed alone; an E that cannot be allocated ends the record ("E": "out of memory").
For information, on the same matrix and N: "spmm_softagg" = torch_op.spmm_softagg(A, B, t), the scalar-weighted messages val[e] * B[c]
under the same softmax (its backward: the gradients of B and t) -- the fused op without the E stream, i.e. what E and dE cost.
"bytes_per_entry": what the fused forward must at least move per stored entry (4 + 8 N: the column index, a gathered B row and the E
row; 4 + 4 N for "copy"), for reading the times against."""
import argparse

import compare_bench as cb


def main():
    ap = argparse.ArgumentParser()
    cb.add_protocol_args(ap)
    ap.add_argument("--dims", default="16,64")
    ap.add_argument("--ops", default="add_relu,copy")
    args = ap.parse_args()
    import torch
    from sextans_amd import torch_op
    from sextans_amd.edge_softagg import spmm_edge_softagg
    dev = torch.device("cuda", 0)
    A, crow, col, val, M, K, nnz = cb.load_matrix(args.matrix)
    gen = torch.Generator(device=dev).manual_seed(1)
    lens = (crow[1:] - crow[:-1]).long()       # built once, untimed
    col64 = col.long()

    def composition(op, B, E, t):
        P = torch.relu(B[col64] + E) if op == "add_relu" else E   # (nnz, N) messages, materialised
        S = P * t
        m = torch.segment_reduce(S.detach(), "max", lengths=lens, axis=0)   # (only a reference point: no gradient through it)
        W = torch.exp(S - torch.repeat_interleave(m, lens, dim=0, output_size=nnz))
        z = torch.segment_reduce(W, "sum", lengths=lens, axis=0)
        acc = torch.segment_reduce(W * P, "sum", lengths=lens, axis=0)
        return acc / z.clamp(min=1e-30)

    extras = ["spmm_softagg"]
    for N in [int(x) for x in args.dims.split(",") if x]:
        B = (torch.rand((K, N), device=dev, generator=gen) * 2 - 1).requires_grad_()
        t = (torch.rand((N,), device=dev, generator=gen) * 4 - 1).requires_grad_()   # temperatures in [-1, 3)
        G = torch.rand((M, N), device=dev, generator=gen) * 2 - 1
        try:
            E = torch.rand((nnz, N), device=dev, generator=gen).mul_(2).sub_(1).requires_grad_()
        except torch.OutOfMemoryError:
            torch.cuda.empty_cache()
            cb.emit({"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "E": "out of memory", "E_bytes": 4 * nnz * N}, args.out)
            continue
        for op in [x for x in args.ops.split(",") if x]:
            leaves = (E, t) if op == "copy" else (B, E, t)

            def apply(side):
                if side == "fused":
                    return spmm_edge_softagg(A, None if op == "copy" else B, E, op=op, t=t)
                if side == "spmm_softagg":
                    return torch_op.spmm_softagg(A, B, t)
                return composition(op, B, E, t)

            def forward(side):
                with torch.no_grad():
                    apply(side)

            def step(side):
                for x in (B, E, t):
                    x.grad = None
                apply(side).backward(G)

            torch_op.clear_cache()
            rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "op": op, "rounds": args.rounds,
                   "composition_form": "messages materialised, segment_reduce max, exp, sum, weighted sum",
                   "grads": ", ".join(("E", "t") if op == "copy" else ("B", "E", "t")),
                   "bytes_per_entry": {"fused_forward_at_least": 4 + (4 if op == "copy" else 8) * N}}
            if args.tag:
                rec["tag"] = args.tag
            sides = ["fused", "composition"]
            peak = {}
            for side, nbytes in cb.warm_up_peaks(step, (B, E, t), sides + extras, may_fail=["composition"]):
                if nbytes is None:
                    sides.remove("composition")
                    rec["composition"] = "out of memory"
                else:
                    peak[side] = nbytes
                for x in (B, E, t):
                    x.grad = None
                torch.cuda.empty_cache()
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
                for x in (B, E, t):
                    x.grad = None
                torch.cuda.empty_cache()
            cb.emit(rec, args.out)
            torch_op.clear_cache()
        del B, E, G, t, leaves
        torch.cuda.empty_cache()
    if args.out:
        recs = [r for r in cb.read_records(args.out, args.matrix) if "op" in r]
        for name in cb.PASSES:
            cb.summary_line(recs, args.matrix, name, lambda r: "N%d %s" % (r["N"], r["op"]), lambda r: r[name])


if __name__ == "__main__":
    main()
