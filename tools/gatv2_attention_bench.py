"""gatv2_attention against the composition a user can write with the other ops of torch_op -- materialise x_dst[row] + x_src[col] as an
(nnz, H, d) tensor, leaky_relu, multiply by att and sum over d, then row_softmax and spmm once per head, stacked -- on the same commit, the
same process and the same tensors, on one GPU.

    python tools/gatv2_attention_bench.py --matrix config4 --out profiles/gatv2_attention.jsonl     (appends one record per (H, d))
    python tools/gatv2_attention_bench.py --matrix small --heads 1,8 --dims 16,64

Matrices, rounds, "ratio", "spread", "verdict", "peak_bytes" and --tag: tools/compare_bench.py.
The composition's nnz-long row-index vector is built once, outside every timed region; its scores become a sparse_csr matrix on A's
index tensors through a small autograd function of the tool's (torch's constructor differentiates through a dense matrix).  Per (H, d):
the forward alone and forward + backward (gradients of x_dst, x_src and att).
A composition case that cannot be allocated is recorded as such ("composition": "out of memory", with the bytes of ONE (nnz, H, d) fp32
tensor as "composition_edge_tensor_bytes") and the fused side is timed alone.
--fused-only times gatv2_attention alone (for choosing the kernels' entries-in-flight count between two builds, or under a profiler): no
composition, no verdict."""
import argparse

import compare_bench as cb


def main():
    ap = argparse.ArgumentParser()
    cb.add_protocol_args(ap)
    ap.add_argument("--heads", default="1,8")
    ap.add_argument("--dims", default="16,64")
    ap.add_argument("--slope", type=float, default=0.2)
    ap.add_argument("--fused-only", action="store_true", help="time gatv2_attention alone (kernel tuning, profiling): no composition, no verdict")
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

    def composition(xd, xs, att):
        s = (torch.nn.functional.leaky_relu(xd[row] + xs[col64], args.slope) * att).sum(-1)   # (nnz, H, d) materialised, -> (nnz, H)
        outs = []
        for h in range(xs.shape[1]):
            P = torch_op.row_softmax(OnPattern.apply(s[:, h].contiguous()))
            outs.append(torch_op.spmm(P, xs[:, h]))
        return torch.stack(outs, dim=1)

    for H in [int(t) for t in args.heads.split(",") if t]:
        for d in [int(t) for t in args.dims.split(",") if t]:
            xd, xs = (((torch.rand((n, H, d), device=dev, generator=gen) * 2 - 1) * 0.5).requires_grad_() for n in (M, K))
            att = ((torch.rand((H, d), device=dev, generator=gen) * 2 - 1) * 0.5).requires_grad_()
            G = torch.rand((M, H, d), device=dev, generator=gen) * 2 - 1
            params = (xd, xs, att)

            def apply(side):
                return torch_op.gatv2_attention(A, xd, xs, att, negative_slope=args.slope) if side == "fused" else composition(xd, xs, att)

            def forward(side):
                with torch.no_grad():
                    apply(side)

            def step(side):
                for t in params:
                    t.grad = None
                apply(side).backward(G)

            torch_op.clear_cache()
            rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "H": H, "d": d, "slope": args.slope, "rounds": args.rounds}
            if args.tag:
                rec["tag"] = args.tag
            sides = ["fused"] if args.fused_only else ["fused", "composition"]
            peak = {}
            for side, nbytes in cb.warm_up_peaks(step, params, list(sides), may_fail=["composition"]):
                if nbytes is None:
                    sides.remove("composition")
                    rec["composition"] = "out of memory"
                    rec["composition_edge_tensor_bytes"] = nnz * H * d * 4
                else:
                    peak[side] = nbytes
            rec["peak_bytes"] = peak
            rec["value_refreshes_composition"] = torch_op.cache_info()["value_refreshes"]
            for name, fn in (("forward", forward), ("forward_backward", step)):
                ts, reps = cb.alternating_rounds(fn, sides, args)
                rec[name] = cb.pass_block(ts)
                rec[name]["reps"] = reps
            cb.emit(rec, args.out)
            torch_op.clear_cache()
            del xd, xs, att, G, params
            torch.cuda.empty_cache()
    if args.out and not args.fused_only:
        recs = cb.read_records(args.out, args.matrix)
        for name in cb.PASSES:
            cb.summary_line(recs, args.matrix, name, lambda r: "H%d d%d" % (r["H"], r["d"]), lambda r: r[name])


if __name__ == "__main__":
    main()
