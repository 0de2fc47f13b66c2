"""The bf16 edge tensors of edge_op() and spmm_edge() against the same ops with fp32 edge tensors -- what the parent commit offers --
on the same commit, in the same process and on the same matrices, on one GPU.

    python tools/edge_bf16_bench.py --matrix config4 --out profiles/edge_bf16.jsonl     (appends one record per N and case)
    python tools/edge_bf16_bench.py --matrix small --dims 16,64 --cases op_add,op_add_e,op_mul,edge_mul,edge_copy

Matrices, rounds, "ratio", "spread", "verdict", "peak_bytes" and --tag: tools/compare_bench.py; the subject side is "bf16", the other "fp32"
(ratio > 1: bf16 is faster).
Cases: "op_add" (edge_op add, no E), "op_add_e" (with E), "op_mul" (no E); "edge_mul" and "edge_copy" (spmm_edge).
Sides: "bf16" = edge_op_bf16(...) with a bf16 E and a bf16 upstream gradient / spmm_edge with a bf16 E; "fp32" = the
same call of edge_op(), an fp32 E and an fp32 upstream gradient / spmm_edge with an fp32 E.  The fp32 edge tensors are the bf16
ones widened, so both sides compute on the same values; the node operands are fp32 on both.  Per N and case: the forward alone and
forward + backward (all gradients the case has); every operand and upstream gradient is allocated before a side's peak is taken, so
"peak_bytes" is what a step allocates on top: Z and the gradients.  A side whose operands or step cannot be allocated is recorded as
"out of memory" and the other is timed alone.
"bytes_per_entry": what each forward must at least move per stored entry -- the 4-byte column index, a gathered fp32 node row where the
op reads one, and the edge rows in their dtype: edge_op add 4 + 8 N against 4 + 6 N, with E 4 + 12 N against 4 + 8 N, spmm_edge mul
4 + 8 N against 4 + 6 N, copy 4 N against 2 N (no index, no node row).  The x_dst / C row is moved once per row."""
import argparse

import compare_bench as cb

CASES = {"op_add": ("edge_op", "add", False), "op_add_e": ("edge_op", "add", True), "op_mul": ("edge_op", "mul", False),
         "edge_mul": ("spmm_edge", "mul", True), "edge_copy": ("spmm_edge", "copy", True)}


def bytes_per_entry(case, N):
    """-> (fp32, bf16): the forward's least traffic per stored entry"""
    if case == "edge_copy":
        return 4 * N, 2 * N
    if case == "op_add_e":
        return 4 + 12 * N, 4 + 8 * N
    return 4 + 8 * N, 4 + 6 * N


def main():
    ap = argparse.ArgumentParser()
    cb.add_protocol_args(ap)
    ap.add_argument("--dims", default="16,64")
    ap.add_argument("--cases", default=",".join(CASES))
    args = ap.parse_args()
    import torch
    from sextans_amd import torch_op
    from sextans_amd.edge_op import edge_op
    from sextans_amd.edge_op_bf16 import edge_op_bf16
    dev = torch.device("cuda", 0)
    A, crow, col, val, M, K, nnz = cb.load_matrix(args.matrix)
    gen = torch.Generator(device=dev).manual_seed(1)

    def uniform(rows, N, dtype=torch.float32):
        return torch.rand((rows, N), device=dev, generator=gen, dtype=dtype).mul_(2.0).sub_(1.0)

    for N in [int(x) for x in args.dims.split(",") if x]:
        for case in [x for x in args.cases.split(",") if x]:
            family, op, with_e = CASES[case]
            f32, b16 = bytes_per_entry(case, N)
            rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "case": case, "rounds": args.rounds,
                   "bytes_per_entry": {"fp32_forward_at_least": f32, "bf16_forward_at_least": b16}}
            if args.tag:
                rec["tag"] = args.tag
            sides = ["bf16", "fp32"]
            nodes, edge, up = {}, {}, {}       # the node operands (shared), a side's E and its upstream gradient
            try:
                if family == "edge_op":
                    nodes = {"xd": uniform(M, N).requires_grad_(), "xs": uniform(K, N).requires_grad_()}
                    up["bf16"] = uniform(nnz, N, torch.bfloat16)
                elif op != "copy":
                    nodes = {"B": uniform(K, N).requires_grad_()}
                if family == "spmm_edge":
                    up["bf16"] = up["fp32"] = uniform(M, N)
                edge["bf16"] = uniform(nnz, N, torch.bfloat16).requires_grad_() if with_e else None
            except torch.OutOfMemoryError:
                nodes, edge, up = {}, {}, {}
                torch.cuda.empty_cache()
                rec["operands"] = "out of memory"
                cb.emit(rec, args.out)
                continue
            try:                               # the fp32 side's own edge tensors, next to the bf16 ones
                edge["fp32"] = edge["bf16"].detach().float().requires_grad_() if with_e else None
                if family == "edge_op":
                    up["fp32"] = up["bf16"].float()
            except torch.OutOfMemoryError:
                edge.pop("fp32", None)
                torch.cuda.empty_cache()
                sides.remove("fp32")
                rec["fp32"] = "out of memory (operands)"
            leaves = list(nodes.values()) + [e for e in edge.values() if e is not None]

            def apply(side):
                if family == "edge_op":
                    return (edge_op_bf16 if side == "bf16" else edge_op)(A, nodes["xd"], nodes["xs"], edge[side], op=op)
                return torch_op.spmm_edge(A, nodes.get("B"), edge[side], op=op)

            def forward(side):
                with torch.no_grad():
                    apply(side)

            def step(side):
                for x in leaves:
                    x.grad = None
                apply(side).backward(up[side])

            torch_op.clear_cache()
            peak = {}
            for side, nbytes in cb.warm_up_peaks(step, leaves, tuple(sides), may_fail=("fp32",)):
                if nbytes is None:
                    sides.remove(side)
                    rec[side] = "out of memory"
                else:
                    peak[side] = nbytes
                for x in leaves:
                    x.grad = None
                torch.cuda.empty_cache()
            rec["peak_bytes"] = peak
            rec["value_refreshes"] = torch_op.cache_info()["value_refreshes"]
            for name, fn in (("forward", forward), ("forward_backward", step)):
                once, lost = cb.slowest_once_dropping(fn, sides, drop="fp32")
                if lost:
                    rec["fp32"] = "out of memory"
                ts, reps = cb.rounds_at(fn, sides, once, args)
                rec[name] = cb.two_sided(ts["bf16"], ts["fp32"], "bf16", "fp32") if "fp32" in ts else {"bf16": cb.stats(ts["bf16"])}
                rec[name]["reps"] = reps
                for x in leaves:
                    x.grad = None
                torch.cuda.empty_cache()
            cb.emit(rec, args.out)
            torch_op.clear_cache()
            del nodes, edge, up, leaves
            torch.cuda.empty_cache()
    if args.out:
        recs = [r for r in cb.read_records(args.out, args.matrix) if "forward" in r]
        for name in cb.PASSES:
            cb.summary_line(recs, args.matrix, name, lambda r: "N%d %s" % (r["N"], r["case"]), lambda r: r[name], missing="fp32: out of memory")


if __name__ == "__main__":
    main()
