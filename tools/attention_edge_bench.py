"""sparse_attention_edge() -- edge features inside the fused attention -- against the composition the other ops of the same commit allow,
in the same process on the same tensors, on one GPU.

    python tools/attention_edge_bench.py --matrix config4 --out profiles/attention_edge.jsonl     (appends one record per (H, d))
    python tools/attention_edge_bench.py --matrix small --heads 1,8 --dims 16,64

The composition, once per head h (S and P materialised, the edge terms as (nnz,) and (nnz, d) temporaries, autograd through all of it):
    S  = sddmm(A, Q_h, K_h) with (Q_h[row] * Ek_h).sum(-1) added to its values      the key term: a gathered (nnz, d) product
    P  = row_softmax(S, scale)
    O_h = spmm(P, V_h) + spmm_edge(A, None, P.values()[:, None] * Ev_h, op="copy")  the value term: an (nnz, d) message tensor
Matrices: "config4" = gen_csr_device(4 M, 4 M, Poisson(40)), "fem" = gen_fem3d_device(110, 110, 110, 3) (3.99 M rows, 318 M non-zeros),
"powerlaw" = gen_powerlaw_device(1 M, 1 M, 6, 1.2, 400 000), "small" = a 200 k-row config-4 for trying the tool out.
Per (H, d = dv): the forward alone (no autograd graph) and forward + backward (gradients of Q, K, V, edge_key and edge_value), each side
timed between HIP events over --rounds rounds of `reps` calls, the two sides in ALTERNATING rounds after one untimed warm-up step per
side; reps is chosen per record so that a round lasts about --round-ms.  "ratio" = composition median / fused median (> 1: the fused
path is faster), "spread" = (max - min) / median of a side's rounds, "verdict": "fused" / "composition" when that side's slowest round
beats the other's fastest -- a difference larger than the spread between repeats -- else "undecided".  "peak_bytes":
torch.cuda.max_memory_allocated over one forward + backward step of a side, above what was allocated before it.  A case whose operands
(the two (nnz, H, d) edge tensors) or whose step do not fit the device is recorded with "could not be allocated" for that side."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NO_MEMORY = "could not be allocated"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", choices=["config4", "fem", "powerlaw", "small"], default="small")
    ap.add_argument("--heads", default="1,8")
    ap.add_argument("--dims", default="16,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-ms", type=float, default=200.0)
    ap.add_argument("--max-reps", type=int, default=8)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from torch.autograd.function import once_differentiable
    from sextans_amd import api, torch_op
    dev = torch.device("cuda", 0)
    if args.matrix == "fem":
        M = K = 110 ** 3 * 3
        p, i, v, nnz = api.gen_fem3d_device(0, 110, 110, 110, 3, 3)
    elif args.matrix == "powerlaw":
        M = K = 1_000_000
        p, i, v, nnz = api.gen_powerlaw_device(0, M, K, 6, 120, 400_000, 7)
    else:
        M = K = 4_000_000 if args.matrix == "config4" else 200_000
        p, i, v, nnz = api.gen_csr_device(0, M, K, 40.0, 4)
    crow = torch.empty(M + 1, dtype=torch.int32, device=dev); col = torch.empty(nnz, dtype=torch.int32, device=dev)
    val = torch.empty(nnz, dtype=torch.float32, device=dev)
    for dst, src, n in ((crow, p, (M + 1) * 4), (col, i, nnz * 4), (val, v, nnz * 4)):
        api.device_copy(0, dst.data_ptr(), src, n)
        api.device_free(0, src)
    A = torch.sparse_csr_tensor(crow, col, val, size=(M, K))
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

    def timed(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / reps   # us per call

    def stats(ts):
        med = statistics.median(ts)
        return {"median_us": med, "min_us": min(ts), "max_us": max(ts), "spread": (max(ts) - min(ts)) / med}

    def compare(f, c):
        r = {"fused": stats(f), "composition": stats(c)}
        r["ratio"] = r["composition"]["median_us"] / r["fused"]["median_us"]
        r["verdict"] = "fused" if max(f) < min(c) else "composition" if max(c) < min(f) else "undecided"
        return r

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    for H in [int(t) for t in args.heads.split(",") if t]:
        for d in [int(t) for t in args.dims.split(",") if t]:
            rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": int(nnz), "H": H, "d": d, "rounds": args.rounds}
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
                emit(rec)
                continue
            leaves = (Q, Kk, V, Ek, Ev)
            scale = d ** -0.5

            def run(fused):
                if fused:
                    return torch_op.sparse_attention_edge(A, Q, Kk, V, edge_key=Ek, edge_value=Ev, scale=scale)
                return composed(Q, Kk, V, Ek, Ev, scale)

            def forward(fused):
                with torch.no_grad():
                    run(fused)

            def step(fused):
                for t in leaves:
                    t.grad = None
                run(fused).backward(G)

            peak, fits = {}, {}
            for fused in (True, False):   # warm-up, and the peak of one step
                side = "fused" if fused else "composition"
                try:
                    step(fused)
                    for t in leaves:
                        t.grad = None
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats(dev)
                    base = torch.cuda.memory_allocated(dev)
                    step(fused)
                    torch.cuda.synchronize()
                    peak[side] = int(torch.cuda.max_memory_allocated(dev) - base)
                    fits[side] = True
                except torch.cuda.OutOfMemoryError:
                    for t in leaves:
                        t.grad = None
                    torch.cuda.empty_cache()
                    peak[side], fits[side] = NO_MEMORY, False
            rec["peak_bytes"] = peak
            for name, fn in (("forward", forward), ("forward_backward", step)):
                sides = [s for s in (True, False) if fits["fused" if s else "composition"] or name == "forward"]
                if not sides:
                    rec[name] = NO_MEMORY
                    continue
                try:
                    once = max(timed(lambda: fn(s), 1) for s in sides)
                    reps = int(max(1, min(args.max_reps, args.round_ms * 1e3 / once)))
                    ts = {s: [] for s in sides}
                    for _ in range(args.rounds):   # alternating rounds
                        for s in sides:
                            ts[s].append(timed(lambda: fn(s), reps))
                except torch.cuda.OutOfMemoryError:
                    torch.cuda.empty_cache()
                    rec[name] = NO_MEMORY
                    continue
                if len(sides) == 2:
                    rec[name] = compare(ts[True], ts[False])
                else:   # one side alone fits: its times, no ratio
                    rec[name] = {("fused" if s else "composition"): stats(t) for s, t in ts.items()}
                    rec[name].update({("composition" if s else "fused"): NO_MEMORY for s in sides}, verdict="fused" if sides == [True] else "composition")
                rec[name]["reps"] = reps
            emit(rec)
            torch_op.clear_cache()
            del Q, Kk, V, Ek, Ev, G, leaves
            torch.cuda.empty_cache()
    if args.out:   # per workload: does the fused path beat the composition by more than the spread between repeats?
        with open(args.out) as fh:
            recs = [r for r in map(json.loads, fh) if r["matrix"] == args.matrix]
        for name in ("forward", "forward_backward"):
            verdicts = ["H%d d%d %s" % (r["H"], r["d"], ("%s x%.2f" % (r[name]["verdict"], r[name]["ratio"])) if isinstance(r.get(name), dict) and "ratio" in r[name]
                        else r.get("operands") or (r[name]["verdict"] + " alone fits" if isinstance(r.get(name), dict) else r.get(name))) for r in recs]
            print("%s %s: %s" % (args.matrix, name, "; ".join(str(x) for x in verdicts)))


if __name__ == "__main__":
    main()
