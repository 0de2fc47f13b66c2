"""The bf16 edge tensors of the gated aggregation (spmm_gated() with a bf16 E, gated_bf16.spmm_gated_bf16()) against the same calls with
the same edge tensors widened to fp32 -- what the parent commit runs on a bf16 operand, less its casts -- on the same commit, in the
same process and on the same matrices, on one GPU.

    python tools/gated_bf16_bench.py --matrix config4 --out profiles/gated_bf16.jsonl     (appends one record per N and case)
    python tools/gated_bf16_bench.py --matrix small --dims 16,64 --cases sum_e,norm_e,gcn

Matrices, rounds, "ratio", "spread", "verdict", "peak_bytes" and --tag: tools/compare_bench.py; the subject side is "bf16", the other "fp32"
(ratio > 1: bf16 is faster).
Cases: "sum_e" and "norm_e" (spmm_gated(A, x_dst, x_src, V, E), ResGatedGraphConv's sum and GatedGCN's normalised one, no z: the route
spmm_gated takes by itself); "gcn" (the GatedGCN layer: normalize=True, E, the z output, and a loss that takes both outputs, so that the
backward reads an upstream gradient of z: spmm_gated_bf16(..., return_edge=True) against spmm_gated(..., E.float(), return_edge=True)).
Sides: "bf16" = E (and in "gcn" z, its upstream gradient and dE) in bf16 through the bf16 entry points; "fp32" = the same call with those
tensors widened (.float()), which takes the fp32 entry points: both sides compute on the same values, the node operands and the upstream
gradient of C are fp32 on both.  Per N and case: the forward alone and forward + backward (all four gradients).  The bf16 side is warmed up
and its peak taken BEFORE the fp32 side's operands exist, so that a step that fits only without them is recorded as running
("bf16_runs_alone"); a side whose operands or step cannot be allocated is recorded as "out of memory", its operands are freed and the other
is timed alone.  Every operand and upstream gradient is allocated before a side's peak is taken, so "peak_bytes" is what a step allocates
on top: C, den, z and the gradients.
"bytes_per_entry": what each forward must at least move per stored entry -- the 4-byte column index, the gathered fp32 rows of x_src and V,
and the edge rows in their dtype: without z 4 + 12 N against 4 + 10 N, with z 4 + 16 N against 4 + 12 N.  x_dst, C and den are moved once
per row."""
import argparse

import compare_bench as cb

CASES = {"sum_e": (False, False), "norm_e": (True, False), "gcn": (True, True)}   # normalize, the z output


def bytes_per_entry(case, N):
    """-> (fp32, bf16): the forward's least traffic per stored entry"""
    return (4 + 16 * N, 4 + 12 * N) if CASES[case][1] else (4 + 12 * N, 4 + 10 * N)


def main():
    ap = argparse.ArgumentParser()
    cb.add_protocol_args(ap)
    ap.add_argument("--dims", default="16,64")
    ap.add_argument("--cases", default=",".join(CASES))
    args = ap.parse_args()
    import torch
    from sextans_amd import torch_op
    from sextans_amd.gated import spmm_gated
    from sextans_amd.gated_bf16 import spmm_gated_bf16
    dev = torch.device("cuda", 0)
    A, crow, col, val, M, K, nnz = cb.load_matrix(args.matrix)
    gen = torch.Generator(device=dev).manual_seed(1)

    def uniform(rows, N, dtype=torch.float32):
        return torch.rand((rows, N), device=dev, generator=gen, dtype=dtype).mul_(2.0).sub_(1.0)

    for N in [int(x) for x in args.dims.split(",") if x]:
        for case in [x for x in args.cases.split(",") if x]:
            normalize, with_z = CASES[case]
            f32, b16 = bytes_per_entry(case, N)
            rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "case": case, "rounds": args.rounds,
                   "bytes_per_entry": {"fp32_forward_at_least": f32, "bf16_forward_at_least": b16}}
            if args.tag:
                rec["tag"] = args.tag
            sides = ["bf16", "fp32"]
            nodes, edge, up = {}, {"bf16": {}, "fp32": {}}, {"bf16": {}, "fp32": {}}   # node operands (shared); a side's E; a side's Gz
            try:
                G = uniform(M, N)
                nodes["x_dst"], nodes["x_src"], nodes["V"] = uniform(M, N).requires_grad_(), uniform(K, N).requires_grad_(), uniform(K, N).requires_grad_()
                edge["bf16"]["E"] = uniform(nnz, N, torch.bfloat16).requires_grad_()
                if with_z:
                    up["bf16"]["Gz"] = uniform(nnz, N, torch.bfloat16)
            except torch.OutOfMemoryError:
                nodes, edge, up, G = {}, {}, {}, None
                torch.cuda.empty_cache()
                rec["operands"] = "out of memory"
                cb.emit(rec, args.out)
                continue

            def leaves():
                return list(nodes.values()) + [x for side in edge.values() for x in side.values()]

            def clear():
                for x in leaves():
                    x.grad = None

            def apply(side):
                """-> the outputs a loss takes: (C,) or (C, z)"""
                E = edge[side]["E"]
                if not with_z:
                    return (spmm_gated(A, nodes["x_dst"], nodes["x_src"], nodes["V"], E, normalize=normalize),)
                op = spmm_gated_bf16 if side == "bf16" else spmm_gated
                return op(A, nodes["x_dst"], nodes["x_src"], nodes["V"], E, normalize=normalize, return_edge=True)

            def forward(side):
                with torch.no_grad():
                    apply(side)

            def step(side):
                clear()
                torch.autograd.backward(list(apply(side)), [G] + list(up[side].values()))

            def drop_fp32(why):
                """the fp32 side leaves: its operands are freed, the bf16 side goes on alone"""
                if "fp32" in sides:
                    sides.remove("fp32")
                edge["fp32"], up["fp32"] = {}, {}
                clear()
                torch.cuda.empty_cache()
                rec["fp32"] = why

            torch_op.clear_cache()
            peak = {}
            # the bf16 side alone first: does its step run on this device, and what does it allocate
            try:
                peak["bf16"] = cb.peak_of_step(lambda: step("bf16"), leaves())
                rec["bf16_runs_alone"] = True
            except torch.OutOfMemoryError:
                clear()
                torch.cuda.empty_cache()
                rec["bf16_runs_alone"] = False
                rec["bf16"] = "out of memory"
                sides.remove("bf16")
            clear()
            torch.cuda.empty_cache()
            try:                               # the fp32 side's own edge tensors, next to the bf16 ones
                edge["fp32"] = {k: x.detach().float().requires_grad_() for k, x in edge["bf16"].items()}
                up["fp32"] = {k: x.float() for k, x in up["bf16"].items()}
                peak["fp32"] = cb.peak_of_step(lambda: step("fp32"), leaves())
            except torch.OutOfMemoryError:
                drop_fp32("out of memory")
            clear()
            torch.cuda.empty_cache()
            rec["peak_bytes"] = peak
            rec["value_refreshes"] = torch_op.cache_info()["value_refreshes"]
            if "bf16" not in sides:            # nothing to compare
                cb.emit(rec, args.out)
                torch_op.clear_cache()
                del nodes, edge, up, G
                torch.cuda.empty_cache()
                continue
            for name, fn in (("forward", forward), ("forward_backward", step)):
                try:
                    once = cb.slowest_once(fn, sides)
                except torch.OutOfMemoryError:     # with both sides' operands resident a step does not fit: bf16 alone
                    drop_fp32("out of memory (next to the bf16 operands)")
                    once = cb.slowest_once(fn, sides)
                ts, reps = cb.rounds_at(fn, sides, once, args)
                rec[name] = cb.two_sided(ts["bf16"], ts["fp32"], "bf16", "fp32") if "fp32" in ts else {"bf16": cb.stats(ts["bf16"])}
                rec[name]["reps"] = reps
                clear()
                torch.cuda.empty_cache()
            cb.emit(rec, args.out)
            torch_op.clear_cache()
            del nodes, edge, up, G
            torch.cuda.empty_cache()
    if args.out:
        recs = [r for r in cb.read_records(args.out, args.matrix) if "forward" in r]
        for name in cb.PASSES:
            cb.summary_line(recs, args.matrix, name, lambda r: "N%d %s" % (r["N"], r["case"]), lambda r: r[name], missing="fp32: out of memory")


if __name__ == "__main__":
    main()
