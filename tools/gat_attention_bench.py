"""gat_attention against the composition a user can write with the other ops of torch_op -- gather a_dst[row] + a_src[col] into an
(nnz, H) array, leaky_relu, then row_softmax and spmm once per head, stacked -- on the same commit, the same process and the same tensors,
on one GPU.

    python tools/gat_attention_bench.py --matrix config4 --out profiles/gat_attention.jsonl     (appends one record per (H, dv))
    python tools/gat_attention_bench.py --matrix small --heads 1,8 --dims 16,64

Matrices, rounds, "ratio", "spread", "verdict", "peak_bytes" and --tag: tools/compare_bench.py.
The composition's nnz-long row-index vector is built once, outside every timed region; its scores become a sparse_csr matrix on A's
index tensors through a small autograd function of the tool's (torch's constructor differentiates through a dense matrix).  Per (H, dv): the
forward alone and forward + backward (gradients of a_dst, a_src and V).
--fused-only times gat_attention alone (for choosing the kernels' entries-in-flight count between two builds): no composition, no verdict."""
import argparse

import compare_bench as cb


def main():
    ap = argparse.ArgumentParser()
    cb.add_protocol_args(ap)
    ap.add_argument("--heads", default="1,8")
    ap.add_argument("--dims", default="16,64")
    ap.add_argument("--slope", type=float, default=0.2)
    ap.add_argument("--fused-only", action="store_true", help="time gat_attention alone (kernel tuning): no composition, no verdict")
    args = ap.parse_args()
    import torch
    from sextans_amd import torch_op
    dev = torch.device("cuda", 0)
    A, crow, col, val, M, K, nnz = cb.load_matrix(args.matrix)
    gen = torch.Generator(device=dev).manual_seed(1)
    row = torch.repeat_interleave(torch.arange(M, device=dev), (crow[1:] - crow[:-1]).long(), output_size=nnz)   # built once, untimed
    col64 = col.long()

    class OnPattern(torch.autograd.Function):
        """nnz values -> the sparse_csr matrix on A's index tensors; the gradient is the CSR gradient's values.  (The backward of torch's own
        constructor goes through a dense M x K tensor: not an option at these sizes, so the composition carries these ten lines.)"""

        @staticmethod
        def forward(ctx, values):
            return torch.sparse_csr_tensor(crow, col, values, size=(M, K))

        @staticmethod
        def backward(ctx, g):
            return g.values()

    def composition(ad, as_, V):
        s = torch.nn.functional.leaky_relu(ad[row] + as_[col64], args.slope)   # (nnz, H)
        outs = []
        for h in range(V.shape[1]):
            P = torch_op.row_softmax(OnPattern.apply(s[:, h].contiguous()))
            outs.append(torch_op.spmm(P, V[:, h]))
        return torch.stack(outs, dim=1)

    for H in [int(t) for t in args.heads.split(",") if t]:
        for d in [int(t) for t in args.dims.split(",") if t]:
            ad, as_ = (((torch.rand((n, H), device=dev, generator=gen) * 2 - 1) * 0.5).requires_grad_() for n in (M, K))
            V = ((torch.rand((K, H, d), device=dev, generator=gen) * 2 - 1) * 0.5).requires_grad_()
            G = torch.rand((M, H, d), device=dev, generator=gen) * 2 - 1
            params = (ad, as_, V)

            def apply(side):
                return torch_op.gat_attention(A, ad, as_, V, negative_slope=args.slope) if side == "fused" else composition(ad, as_, V)

            def forward(side):
                with torch.no_grad():
                    apply(side)

            def step(side):
                for t in params:
                    t.grad = None
                apply(side).backward(G)

            torch_op.clear_cache()
            rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "H": H, "dv": d, "slope": args.slope, "rounds": args.rounds}
            if args.tag:
                rec["tag"] = args.tag
            sides = ["fused"] if args.fused_only else ["fused", "composition"]
            rec["peak_bytes"] = dict(cb.warm_up_peaks(step, params, sides))
            rec["kernel_refreshes_composition"] = torch_op.cache_info()["value_refreshes"]
            for name, fn in (("forward", forward), ("forward_backward", step)):
                ts, reps = cb.alternating_rounds(fn, sides, args)
                rec[name] = cb.pass_block(ts)
                rec[name]["reps"] = reps
            cb.emit(rec, args.out)
            torch_op.clear_cache()
            del ad, as_, V, G, params
    if args.out and not args.fused_only:
        recs = cb.read_records(args.out, args.matrix)
        for name in cb.PASSES:
            cb.summary_line(recs, args.matrix, name, lambda r: "H%d dv%d" % (r["H"], r["dv"]), lambda r: r[name])


if __name__ == "__main__":
    main()
