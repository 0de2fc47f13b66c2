"""score_attention against what a user can write without it, on the same commit, the same process and the same tensors, on one GPU:

  (a) "per_head"  the composition the project's other ops allow: per head, row_softmax -> spmm on a sparse_csr matrix that carries the
                  head's scores as values requiring grad, stacked;
  (b) "torch"     torch's own composition: segment_reduce max / sum softmax over the (nnz, H) scores, V[col] materialised as
                  (nnz, H, dv), segment_reduce sum.  Skipped (and recorded as skipped, with the bytes it would need) where the
                  materialised messages do not fit;
  (c) "gat"       gat_attention fed the a_dst / a_src that produce the same scores, S = leaky_relu(a_dst[row] + a_src[col]): what reading
                  S costs against recomputing it from 2 floats per node.

    python tools/score_attention_bench.py --matrix config4 --out profiles/score_attention.jsonl     (appends one record per (H, dv))
    python tools/score_attention_bench.py --matrix small --heads 1,8 --dims 16,64

Matrices, rounds, "ratio", "spread", "verdict", "peak_bytes" and --tag: tools/compare_bench.py; each other side is compared with the fused
op in rounds of its own, with "fused" / the other side's name as the verdict's words, and reps is chosen per comparison.
The nnz-long row-index vector and the scores are built once, outside every timed region.  Per (H, dv) and other side: the forward alone
and forward + backward (gradients of S -- for (c) of a_dst and a_src -- and V).
--passes times the kernels alone through the C ABI -- the forward, the backward's row pass (d_dV NULL), its column pass (d_dS NULL) and
both -- and writes records of "kind": "passes" (keep them in a file of their own: profiles/score_attention_passes.jsonl)."""
import argparse

import compare_bench as cb

SIDES = ("per_head", "torch", "gat")


def main():
    ap = argparse.ArgumentParser()
    cb.add_protocol_args(ap)
    ap.add_argument("--heads", default="1,8")
    ap.add_argument("--dims", default="16,64")
    ap.add_argument("--sides", default=",".join(SIDES))
    ap.add_argument("--slope", type=float, default=0.2)
    ap.add_argument("--passes", action="store_true", help="time the forward, the row pass, the column pass and the backward on the C ABI: no other side")
    args = ap.parse_args()
    sides = [s for s in args.sides.split(",") if s]
    assert all(s in SIDES for s in sides), sides
    import torch
    from sextans_amd import api, torch_op
    dev = torch.device("cuda", 0)
    A, crow, col, val, M, K, nnz = cb.load_matrix(args.matrix)
    gen = torch.Generator(device=dev).manual_seed(1)
    row = torch_op.entry_rows(A)   # built once, untimed
    col64 = col.long()
    lengths = (crow[1:] - crow[:-1]).long()

    class OnPattern(torch.autograd.Function):
        """nnz values -> the sparse_csr matrix on A's index tensors; the gradient is the CSR gradient's values.  (The backward of torch's own
        constructor goes through a dense M x K tensor: not an option at these sizes.)"""

        @staticmethod
        def forward(ctx, values):
            return torch.sparse_csr_tensor(crow, col, values, size=(M, K))

        @staticmethod
        def backward(ctx, g):
            return g.values()

    def per_head(S, V):
        outs = []
        for h in range(V.shape[1]):
            P = torch_op.row_softmax(OnPattern.apply(S[:, h].contiguous()))
            outs.append(torch_op.spmm(P, V[:, h]))
        return torch.stack(outs, dim=1)

    def torch_own(S, V):
        m = torch.segment_reduce(S.detach(), "max", lengths=lengths, axis=0, unsafe=True)
        e = torch.exp(S - m[row])
        z = torch.segment_reduce(e, "sum", lengths=lengths, axis=0, unsafe=True)
        P = e / z[row]
        msg = (P[:, :, None] * V[col64]).flatten(1)
        return torch.segment_reduce(msg, "sum", lengths=lengths, axis=0, unsafe=True).unflatten(1, V.shape[1:])

    def passes(H, d):
        """the C ABI directly: the forward, the row pass alone (d_dV NULL), the column pass alone (d_dS NULL) and the whole backward"""
        S = torch.rand((nnz, H), device=dev, generator=gen) * 2 - 1
        V = (torch.rand((K, H, d), device=dev, generator=gen) * 2 - 1) * 0.5
        G = torch.rand((M, H, d), device=dev, generator=gen) * 2 - 1
        torch_op.clear_cache()
        torch_op.score_attention(A, S.clone().requires_grad_(), V.clone().requires_grad_()).backward(G)   # warm-up: engine, tables, A^T
        eng = next(iter(torch_op._cache.values())).eng
        O, lse = torch.empty((M, H, d), device=dev), torch.empty((M, H), device=dev)
        dS, dV = torch.empty((nnz, H), device=dev), torch.empty((K, H, d), device=dev)
        st = torch.cuda.current_stream().cuda_stream

        def fwd():
            eng.score_attention_device(api.SCORE_SOFTMAX, H, d, S.data_ptr(), H, V.data_ptr(), H * d, O.data_ptr(), H * d, lse.data_ptr(), None, st)

        def bwd(rows, cols):
            eng.score_attention_backward_device(api.SCORE_SOFTMAX, H, d, S.data_ptr(), H, V.data_ptr(), H * d, O.data_ptr(), H * d, lse.data_ptr(),
                                                G.data_ptr(), H * d, dS.data_ptr() if rows else None, H, dV.data_ptr() if cols else None, H * d,
                                                None, st)

        fwd()
        rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "H": H, "dv": d, "rounds": args.rounds, "kind": "passes"}
        for name, fn in (("forward", fwd), ("row_pass", lambda: bwd(True, False)), ("column_pass", lambda: bwd(False, True)),
                         ("backward", lambda: bwd(True, True))):
            ts, _ = cb.alternating_rounds(lambda f: f(), [fn], args)   # (one side, itself the call)
            rec[name] = cb.stats(ts[fn])
        torch_op.clear_cache()
        return rec

    if args.passes:
        for H in [int(t) for t in args.heads.split(",") if t]:
            for d in [int(t) for t in args.dims.split(",") if t]:
                cb.emit(passes(H, d), args.out)
        return

    for H in [int(t) for t in args.heads.split(",") if t]:
        for d in [int(t) for t in args.dims.split(",") if t]:
            ad, as_ =(((torch.rand((n, H), device=dev, generator=gen) * 2 - 1) * 0.5).requires_grad_() for n in (M, K))
            V = ((torch.rand((K, H, d), device=dev, generator=gen) * 2 - 1) * 0.5).requires_grad_()
            G = torch.rand((M, H, d), device=dev, generator=gen) * 2 - 1
            with torch.no_grad():
                S = torch.nn.functional.leaky_relu(ad[row] + as_[col64], args.slope)   # the scores gat_attention computes, untimed
            S.requires_grad_()
            params = {"fused": (S, V), "per_head": (S, V), "torch": (S, V), "gat": (ad, as_, V)}

            def apply(side):
                if side == "fused":
                    return torch_op.score_attention(A, S, V)
                if side == "per_head":
                    return per_head(S, V)
                if side == "torch":
                    return torch_own(S, V)
                return torch_op.gat_attention(A, ad, as_, V, negative_slope=args.slope)

            def forward(side):
                with torch.no_grad():
                    apply(side)

            def step(side):
                for t in params[side]:
                    t.grad = None
                apply(side).backward(G)

            torch_op.clear_cache()
            rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "H": H, "dv": d, "slope": args.slope, "rounds": args.rounds}
            if args.tag:
                rec["tag"] = args.tag
            run, peak = [], {}
            for side in ["fused"] + sides:   # warm-up, and the peak of one step
                if side == "torch":
                    free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
                    need = 4 * nnz * H * d * 4   # the messages, their gradient, V[col] and its gradient
                    if need > 0.8 * free:
                        rec["torch_skipped"] = {"needs_bytes": need, "free_bytes": int(free)}
                        continue
                    try:
                        step(side)
                    except RuntimeError as err:   # (out of memory after all, or a segment_reduce this torch build lacks)
                        rec["torch_skipped"] = {"error": str(err).splitlines()[0][:200]}
                        for t in params[side]:
                            t.grad = None
                        torch.cuda.empty_cache()
                        continue
                peak[side] = cb.peak_of_step(lambda: step(side), params[side])
                for t in params[side]:
                    t.grad = None
                torch.cuda.empty_cache()
                if side != "fused":
                    run.append(side)
            rec["peak_bytes"] = peak
            rec["value_refreshes_per_head"] = torch_op.cache_info()["value_refreshes"]
            for name, fn in (("forward", forward), ("forward_backward", step)):
                rec[name] = {}
                for side in run:
                    ts, reps = cb.alternating_rounds(fn, ["fused", side], args)
                    rec[name][side] = cb.two_sided(ts["fused"], ts[side], "fused", side)
                    rec[name][side]["reps"] = reps
            cb.emit(rec, args.out)
            torch_op.clear_cache()
            del ad, as_, V, G, S, params
            torch.cuda.empty_cache()
    if args.out:
        recs = cb.read_records(args.out, args.matrix)
        for name in cb.PASSES:
            for side in sides:
                cb.summary_line([r for r in recs if side in r[name]], args.matrix, "%s vs %s" % (name, side),
                                lambda r: "H%d dv%d" % (r["H"], r["dv"]), lambda r: r[name][side])


if __name__ == "__main__":
    main()
