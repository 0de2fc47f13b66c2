"""sparse_attention(fused=True) against sparse_attention(fused=False) -- the composition sddmm -> row_softmax -> spmm, once per head -- on
the same commit, the same process and the same tensors, on one GPU.

    python tools/fused_attention_bench.py --matrix config4 --out profiles/fused_attention.jsonl     (appends one record per (H, d))
    python tools/fused_attention_bench.py --matrix small --heads 1,8 --dims 16,64

Matrices, rounds, "ratio", "spread", "verdict" and "peak_bytes": tools/compare_bench.py.
Per (H, d = dv): the forward alone and forward + backward (gradients of Q, K and V)."""
import argparse

import compare_bench as cb


def main():
    ap = argparse.ArgumentParser()
    cb.add_protocol_args(ap, tag=False)
    ap.add_argument("--heads", default="1,8")
    ap.add_argument("--dims", default="16,64")
    args = ap.parse_args()
    import torch
    from sextans_amd import torch_op
    dev = torch.device("cuda", 0)
    A, crow, col, val, M, K, nnz = cb.load_matrix(args.matrix)
    gen = torch.Generator(device=dev).manual_seed(1)

    for H in [int(t) for t in args.heads.split(",") if t]:
        for d in [int(t) for t in args.dims.split(",") if t]:
            Q, Kk, V = (((torch.rand((n, H, d), device=dev, generator=gen) * 2 - 1) * 0.5).requires_grad_() for n in (M, K, K))
            G = torch.rand((M, H, d), device=dev, generator=gen) * 2 - 1

            def forward(side):
                with torch.no_grad():
                    torch_op.sparse_attention(A, Q, Kk, V, fused=side == "fused")

            def step(side):
                for t in (Q, Kk, V):
                    t.grad = None
                torch_op.sparse_attention(A, Q, Kk, V, fused=side == "fused").backward(G)

            torch_op.clear_cache()
            rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "H": H, "d": d, "rounds": args.rounds}
            sides = ("fused", "composition")
            rec["peak_bytes"] = dict(cb.warm_up_peaks(step, (Q, Kk, V), sides))
            rec["kernel_refreshes_composition"] = torch_op.cache_info()["value_refreshes"]
            for name, fn in (("forward", forward), ("forward_backward", step)):
                ts, reps = cb.alternating_rounds(fn, sides, args)
                rec[name] = cb.two_sided(ts["fused"], ts["composition"])
                rec[name]["reps"] = reps
            cb.emit(rec, args.out)
            torch_op.clear_cache()
            del Q, Kk, V, G
    if args.out:
        recs = cb.read_records(args.out, args.matrix)
        for name in cb.PASSES:
            cb.summary_line(recs, args.matrix, name, lambda r: "H%d d%d" % (r["H"], r["d"]), lambda r: r[name])


if __name__ == "__main__":
    main()
