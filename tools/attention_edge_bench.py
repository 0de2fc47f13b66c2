"""sparse_attention_edge() -- edge features inside the fused attention -- against the composition the other ops of the same commit allow,
in the same process on the same tensors, on one GPU.

    python tools/attention_edge_bench.py --matrix config4 --out profiles/attention_edge.jsonl     (appends one record per (H, d))
    python tools/attention_edge_bench.py --matrix small --heads 1,8 --dims 16,64

The composition, once per head h (S and P materialised, the edge terms as (nnz,) and (nnz, d) temporaries, autograd through all of it):
    S  = sddmm(A, Q_h, K_h) with (Q_h[row] * Ek_h).sum(-1) added to its values      the key term: a gathered (nnz, d) product
    P  = row_softmax(S, scale)
    O_h = spmm(P, V_h) + spmm_edge(A, None, P.values()[:, None] * Ev_h, op="copy")  the value term: an (nnz, d) message tensor
Matrices, rounds, "ratio", "spread", "verdict" and "peak_bytes": tools/compare_bench.py.
Per (H, d = dv): the forward alone and forward + backward (gradients of Q, K, V, edge_key and edge_value).  A case whose operands (the
two (nnz, H, d) edge tensors) or whose step do not fit the device is recorded with "could not be allocated" for that side."""
import argparse

import compare_bench as cb

NO_MEMORY = "could not be allocated"


def main():
    ap = argparse.ArgumentParser()
    cb.add_protocol_args(ap, tag=False)
    ap.add_argument("--heads", default="1,8")
    ap.add_argument("--dims", default="16,64")
    args = ap.parse_args()
    import torch
    from torch.autograd.function import once_differentiable
    from sextans_amd import torch_op
    dev = torch.device("cuda", 0)
    A, crow, col, val, M, K, nnz = cb.load_matrix(args.matrix)
    row = torch.repeat_interleave(torch.arange(M, device=dev, dtype=torch.int32), (crow[1:] - crow[:-1]).long()).long()   # the composition's gather index
    gen = torch.Generator(device=dev).manual_seed(1)

    class AddToValues(torch.autograd.Function):
        """S with `extra` (nnz,) added to its values, on S's own index tensors"""

        @staticmethod
        def forward(ctx, S, extra):
            c, r = torch_op._index_tensors(S)
            ctx.save_for_backward(c, r)
            ctx.shape = tuple(S.shape)
            return torch.sparse_csr_tensor(c, r, S.values().detach() + extra, size=ctx.shape)

        @staticmethod
        @once_differentiable
        def backward(ctx, G):
            c, r = ctx.saved_tensors
            g = torch_op._grad_values(G, c, r, int(r.numel()))
            return torch.sparse_csr_tensor(c, r, g, size=ctx.shape), g

    class Split(torch.autograd.Function):
        """P -> (P again, P's values as a dense (nnz,) tensor): the SpMM takes the one, the edge messages the other, and ONE gradient
        on the pattern comes back (autograd would otherwise have to add two sparse gradients)"""

        @staticmethod
        def forward(ctx, P):
            c, r = torch_op._index_tensors(P)
            ctx.save_for_backward(c, r)
            ctx.shape = tuple(P.shape)
            ctx.set_materialize_grads(False)
            vals = P.values().detach()
            return torch.sparse_csr_tensor(c, r, vals, size=ctx.shape), vals.clone()

        @staticmethod
        @once_differentiable
        def backward(ctx, Gs, gv):
            c, r = ctx.saved_tensors
            g = torch_op._grad_values(Gs, c, r, int(r.numel())) if Gs is not None else None
            if gv is not None:
                g = gv if g is None else g + gv
            return torch.sparse_csr_tensor(c, r, g.contiguous(), size=ctx.shape)

    def composed(Q, Kk, V, Ek, Ev, scale):
        outs = []
        for h in range(Q.shape[1]):
            S = torch_op.sddmm(A, Q[:, h], Kk[:, h])
            c, r = torch_op._index_tensors(S)
            S = torch_op._carry(AddToValues.apply(S, (Q[:, h][row] * Ek[:, h]).sum(-1)), c, r)
            P, pv = Split.apply(torch_op.row_softmax(S, scale))
            P = torch_op._carry(P, c, r)
            outs.append(torch_op.spmm(P, V[:, h]) + torch_op.spmm_edge(A, None, pv[:, None] * Ev[:, h], op="copy"))
        return torch.stack(outs, dim=1)

    for H in [int(t) for t in args.heads.split(",") if t]:
        for d in [int(t) for t in args.dims.split(",") if t]:
            rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "H": H, "d": d, "rounds": args.rounds}
            torch_op.clear_cache()
            try:
                # (filled in place: no temporaries of the operands' size)
                Q, Kk, V = (torch.empty((n, H, d), device=dev).uniform_(-0.5, 0.5, generator=gen).requires_grad_() for n in (M, K, K))
                Ek, Ev = (torch.empty((nnz, H, d), device=dev).uniform_(-0.5, 0.5, generator=gen).requires_grad_() for _ in range(2))
                G = torch.empty((M, H, d), device=dev).uniform_(-1.0, 1.0, generator=gen)
            except torch.cuda.OutOfMemoryError:
                Q = Kk = V = Ek = Ev = G = None
                torch.cuda.empty_cache()
                rec["operands"] = NO_MEMORY
                cb.emit(rec, args.out)
                continue
            leaves = (Q, Kk, V, Ek, Ev)
            scale = d ** -0.5

            def run(side):
                if side == "fused":
                    return torch_op.sparse_attention_edge(A, Q, Kk, V, edge_key=Ek, edge_value=Ev, scale=scale)
                return composed(Q, Kk, V, Ek, Ev, scale)

            def forward(side):
                with torch.no_grad():
                    run(side)

            def step(side):
                for t in leaves:
                    t.grad = None
                run(side).backward(G)

            both = ("fused", "composition")
            peak = {side: NO_MEMORY if nbytes is None else nbytes for side, nbytes in cb.warm_up_peaks(step, leaves, both, may_fail=both)}
            rec["peak_bytes"] = peak
            for name, fn in (("forward", forward), ("forward_backward", step)):
                sides = [s for s in both if peak[s] != NO_MEMORY or name == "forward"]
                if not sides:
                    rec[name] = NO_MEMORY
                    continue
                try:
                    ts, reps = cb.alternating_rounds(fn, sides, args)
                except torch.cuda.OutOfMemoryError:
                    torch.cuda.empty_cache()
                    rec[name] = NO_MEMORY
                    continue
                if len(sides) == 2:
                    rec[name] = cb.two_sided(ts["fused"], ts["composition"])
                else:   # one side alone fits: its times, no ratio
                    rec[name] = {s: cb.stats(t) for s, t in ts.items()}
                    rec[name].update({s: NO_MEMORY for s in both if s not in sides}, verdict=sides[0])
                rec[name]["reps"] = reps
            cb.emit(rec, args.out)
            torch_op.clear_cache()
            del Q, Kk, V, Ek, Ev, G, leaves
            torch.cuda.empty_cache()
    if args.out:
        recs = cb.read_records(args.out, args.matrix)
        for name in cb.PASSES:
            cb.summary_line(recs, args.matrix, name, lambda r: "H%d d%d" % (r["H"], r["d"]),
                            lambda r: r[name] if isinstance(r.get(name), dict) and "ratio" in r[name] else None,
                            lambda r: r.get("operands") or (r[name]["verdict"] + " alone fits" if isinstance(r.get(name), dict) else r.get(name)))


if __name__ == "__main__":
    main()
