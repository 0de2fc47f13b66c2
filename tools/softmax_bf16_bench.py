"""The bf16 edge tensors of vector_attention() and spmm_edge_softagg() against the same ops with the same edge tensors widened to fp32
-- what the parent commit runs on a bf16 operand, less its casts -- on the same commit, in the same process and on the same matrices,
on one GPU.

    python tools/softmax_bf16_bench.py --matrix config4 --out profiles/softmax_bf16.jsonl     (appends one record per N and case)
    python tools/softmax_bf16_bench.py --matrix small --dims 16,64 --cases vatt_node,vatt_add,soft_add_relu,soft_copy

Matrices, rounds, "ratio", "spread", "verdict", "peak_bytes" and --tag: tools/compare_bench.py; the subject side is "bf16", the other "fp32"
(ratio > 1: bf16 is faster).
Cases: "vatt_node" and "vatt_add" (vector_attention(A, S, V) / (A, S, V, D)); "soft_add_relu" and "soft_copy" (spmm_edge_softagg with an
(N,) temperature, GENConv's message and a materialised one).
Sides: "bf16" = the op with bf16 S and D / a bf16 E, which takes the bf16 entry points; "fp32" = the same call with those tensors widened
(.float()), which takes the fp32 entry points: both sides compute on the same values, the node operands, t and the upstream gradient are
fp32 on both.  Per N and case: the forward alone and forward + backward (all gradients the case has).  The bf16 side is warmed up and
its peak taken BEFORE the fp32 side's operands exist, so that a step that fits only without them is recorded as running ("runs_alone");
a side whose operands or step cannot be allocated is recorded as "out of memory", its operands are freed and the other is timed alone.
Every operand and upstream gradient is allocated before a side's peak is taken, so "peak_bytes" is what a step allocates on top: C, lse
and the gradients.
"bytes_per_entry": what each forward must at least move per stored entry -- the 4-byte column index, a gathered fp32 node row where the
op reads one, and the edge rows in their dtype: vector attention node 4 + 8 N against 4 + 6 N, add 4 + 12 N against 4 + 8 N; edge
softagg add_relu 4 + 8 N against 4 + 6 N, copy 4 N against 2 N (no index, no node row).  C and lse are moved once per row."""
import argparse

import compare_bench as cb

CASES = {"vatt_node": ("vatt", "node"), "vatt_add": ("vatt", "add"), "soft_add_relu": ("soft", "add_relu"), "soft_copy": ("soft", "copy")}


def bytes_per_entry(case, N):
    """-> (fp32, bf16): the forward's least traffic per stored entry"""
    if case == "soft_copy":
        return 4 * N, 2 * N
    if case == "vatt_add":
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
    from sextans_amd.edge_softagg import spmm_edge_softagg
    from sextans_amd.vector_attention import vector_attention
    dev = torch.device("cuda", 0)
    A, crow, col, val, M, K, nnz = cb.load_matrix(args.matrix)
    gen = torch.Generator(device=dev).manual_seed(1)

    def uniform(rows, N, dtype=torch.float32, scale=1.0):
        return torch.rand((rows, N), device=dev, generator=gen, dtype=dtype).mul_(2.0 * scale).sub_(scale)

    for N in [int(x) for x in args.dims.split(",") if x]:
        for case in [x for x in args.cases.split(",") if x]:
            family, op = CASES[case]
            f32, b16 = bytes_per_entry(case, N)
            rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": nnz, "N": N, "case": case, "rounds": args.rounds,
                   "bytes_per_entry": {"fp32_forward_at_least": f32, "bf16_forward_at_least": b16}}
            if args.tag:
                rec["tag"] = args.tag
            sides = ["bf16", "fp32"]
            nodes, edge = {}, {"bf16": {}, "fp32": {}}    # the node operands, t and G (shared); a side's edge tensors by name
            try:
                G = uniform(M, N)
                if op != "copy":
                    nodes["V"] = uniform(K, N).requires_grad_()
                if family == "soft":
                    nodes["t"] = uniform(1, N)[0].add(1.5).requires_grad_()      # (0.5 .. 2.5)
                    edge["bf16"]["E"] = uniform(nnz, N, torch.bfloat16).requires_grad_()
                else:
                    edge["bf16"]["S"] = uniform(nnz, N, torch.bfloat16, 4.0).requires_grad_()
                    if op == "add":
                        edge["bf16"]["D"] = uniform(nnz, N, torch.bfloat16).requires_grad_()
            except torch.OutOfMemoryError:
                nodes, edge, G = {}, {}, None
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
                e = edge[side]
                if family == "vatt":
                    return vector_attention(A, e["S"], nodes["V"], e.get("D"))
                return spmm_edge_softagg(A, nodes.get("V"), e["E"], op=op, t=nodes["t"])

            def forward(side):
                with torch.no_grad():
                    apply(side)

            def step(side):
                clear()
                apply(side).backward(G)

            def drop_fp32(why):
                """the fp32 side leaves: its operands are freed, the bf16 side goes on alone"""
                if "fp32" in sides:
                    sides.remove("fp32")
                edge["fp32"] = {}
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
                del nodes, edge, G
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
            del nodes, edge, G
            torch.cuda.empty_cache()
    if args.out:
        recs = [r for r in cb.read_records(args.out, args.matrix) if "forward" in r]
        for name in cb.PASSES:
            cb.summary_line(recs, args.matrix, name, lambda r: "N%d %s" % (r["N"], r["case"]), lambda r: r[name], missing="fp32: out of memory")


if __name__ == "__main__":
    main()
