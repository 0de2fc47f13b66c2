"""vector_attention.vector_attention(A, S, V, D) against the composition torch allows on a GPU -- materialise the (nnz, N) messages
(V[col] for "node", V[col] + D for "add"), then torch.segment_reduce max of the scores S over the row lengths, exp, segment_reduce sum,
the weighted segment_reduce sum, autograd through it -- on the same commit, the same process and the same tensors, on one GPU.

    python tools/vector_attention_bench.py --matrix config4 --out profiles/vector_attention.jsonl     (appends one record per N and mode)
    python tools/vector_attention_bench.py --matrix small --dims 16,64 --modes node,add

Matrices, rounds, "ratio", "spread", "verdict", "peak_bytes" and --tag: tools/compare_bench.py.
The composition's row lengths and 64-bit column indices are built once, outside every timed region.  Per N and mode: the forward alone
and forward + backward (the gradients of S, of V and -- "add" -- of D); S, V, D, G and the matrix are allocated before a side's peak is
taken.  A composition case that cannot be allocated is recorded as such ("composition": "out of memory") and the fused side is timed
alone; operands that cannot be allocated end the record ("operands": "out of memory"), and so does a fused training step whose gradients
do not fit next to them ("fused": "out of memory").
For information, on the same matrix and N, the sibling without the S stream: "spmm_edge_softagg" = edge_softagg.spmm_edge_softagg(A, V,
D, "add") for "add" (the same messages, the score computed from them: what reading S and writing dS cost), "spmm_softagg" =
torch_op.spmm_softagg(A, V) for "node" (the messages val[e] * V[c]).
"bytes_per_entry": what the fused forward must at least move per stored entry (4 + 8 N: the column index, the S row and a gathered V
row; 4 + 12 N for "add", which reads the D row as well), for reading the times against."""
import argparse

import compare_bench as cb


def main():
    ap = argparse.ArgumentParser()
    cb.add_protocol_args(ap)
    ap.add_argument("--dims", default="16,64")
    ap.add_argument("--modes", default="node,add")
    args = ap.parse_args()
    import torch
    from sextans_amd import torch_op
    from sextans_amd.edge_softagg import spmm_edge_softagg
    from sextans_amd.vector_attention import vector_attention
    dev = torch.device("cuda", 0)
    A, crow, col, val, M, K, nnz = cb.load_matrix(args.matrix)
    gen = torch.Generator(device=dev).manual_seed(1)
    lens = (crow[1:] - crow[:-1]).long()       # built once, untimed
    col64 = col.long()

    def composition(S, V, D):
        P = V[col64] if D is None else V[col64] + D   # (nnz, N) messages, materialised
        m = torch.segment_reduce(S.detach(), "max", lengths=lens, axis=0)   # (only a reference point: no gradient through it)
        W = torch.exp(S - torch.repeat_interleave(m, lens, dim=0, output_size=nnz))
        z = torch.segment_reduce(W, "sum", lengths=lens, axis=0)
        acc = torch.segment_reduce(W * P, "sum", lengths=lens, axis=0)
        return acc / z.clamp(min=1e-30)

    def uniform(rows, N, scale):
        return torch.rand((rows, N), device=dev, generator=gen).mul_(2 * scale).sub_(scale)

    for N in [int(x) for x in args.dims.split(",") if x]:
        for mode in [x for x in args.modes.split(",") if x]:
            S = V = D = G = None
            try:
                V = uniform(K, N, 1.0).requires_grad_()
                G = uniform(M, N, 1.0)
                S = uniform(nnz, N, 4.0).requires_grad_()          # scores in [-4, 4)
                D = uniform(nnz, N, 1.0).requires_grad_() if mode == "add" else None
            except torch.OutOfMemoryError:
                del S, V, D, G
                torch.cuda.empty_cache()
                cb.emit({"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "mode": mode, "operands": "out of memory",
                         "operand_bytes": 4 * N * (K + M + nnz * (2 if mode == "add" else 1))}, args.out)
                continue
            leaves = [x for x in (S, V, D) if x is not None]
            extra = "spmm_edge_softagg" if mode == "add" else "spmm_softagg"

            def apply(side):
                if side == "fused":
                    return vector_attention(A, S, V, D)
                if side == "spmm_edge_softagg":
                    return spmm_edge_softagg(A, V, D, op="add")
                if side == "spmm_softagg":
                    return torch_op.spmm_softagg(A, V)
                return composition(S, V, D)

            def forward(side):
                with torch.no_grad():
                    apply(side)

            def step(side):
                for x in leaves:
                    x.grad = None
                apply(side).backward(G)

            torch_op.clear_cache()
            rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "mode": mode, "rounds": args.rounds,
                   "composition_form": "messages materialised, segment_reduce max, exp, sum, weighted sum",
                   "grads": ", ".join(("S", "V", "D") if mode == "add" else ("S", "V")),
                   "bytes_per_entry": {"fused_forward_at_least": 4 + (12 if mode == "add" else 8) * N}}
            if args.tag:
                rec["tag"] = args.tag
            sides = ["fused", "composition"]
            extras = [extra]
            peak = {}
            for side, nbytes in cb.warm_up_peaks(step, leaves, sides + extras, may_fail=sides + extras):
                if nbytes is None:
                    (sides if side in sides else extras).remove(side)
                    rec[side] = "out of memory"
                else:
                    peak[side] = nbytes
                for x in leaves:
                    x.grad = None
                torch.cuda.empty_cache()
                if "fused" not in sides:   # (the gradients of a training step do not fit next to the operands: nothing to compare)
                    break
            rec["peak_bytes"] = peak
            if "fused" not in sides:
                cb.emit(rec, args.out)
                torch_op.clear_cache()
                del S, V, D, G, leaves
                torch.cuda.empty_cache()
                continue
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
                for x in leaves:
                    x.grad = None
                torch.cuda.empty_cache()
            cb.emit(rec, args.out)
            torch_op.clear_cache()
            del S, V, D, G, leaves
            torch.cuda.empty_cache()
    if args.out:
        recs = [r for r in cb.read_records(args.out, args.matrix) if "forward" in r]
        for name in cb.PASSES:
            cb.summary_line(recs, args.matrix, name, lambda r: "N%d %s" % (r["N"], r["mode"]), lambda r: r[name])


if __name__ == "__main__":
    main()
