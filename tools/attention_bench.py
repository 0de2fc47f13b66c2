"""Row softmax on A's pattern and the sparse attention pipeline against what torch offers without them, on one GPU.

    python tools/attention_bench.py --matrix config4 --out profiles/row_softmax.jsonl          (appends one record per run)
    python tools/attention_bench.py --matrix fem --steps 16,64
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/attention_bench.py --matrix fem --kernels-only

Matrices and "spread": tools/compare_bench.py (this tool takes a fixed --reps, and has no verdict of its own).

Kernel records: sextans_row_softmax_device / _backward_device, median us over --rounds rounds of --reps calls between HIP events, bytes
from shapes (8 nnz + 4 (M + 1) forward, 12 nnz + 4 (M + 1) backward) and their share of the 8 TB/s the project's rooflines use (the
achievable copy figure on this chip is about 6.3 TB/s).
Baseline: what a user can compose from torch ops on the values of a CSR tensor -- scatter_reduce(amax), gather, exp, index_add_, gather,
divide, and torch's autograd of that for the backward; the row-index vector (nnz int64) is built outside the timed region.  Baseline and
engine are timed in the same process in alternating rounds; "ratio" = baseline median / engine median, "spread" = (max - min) / median
of each side's rounds.
Whole-step records (--steps d,...): forward + backward of torch_op.sparse_attention at head dimension d against the same pipeline with
the torch composition in place of row_softmax."""
import argparse
import statistics

import compare_bench as cb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrix", choices=list(cb.MATRICES), default="small")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", default="", help="comma-separated head dimensions for the whole-step record (none: kernels only)")
    ap.add_argument("--kernels-only", action="store_true", help="the two engine kernels alone, no baseline (profiler runs)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from sextans_amd import api, torch_op
    dev = torch.device("cuda", 0)
    crow, col, val, M, K, nnz = cb.load_matrix(args.matrix)[1:]
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand(nnz, device=dev, generator=gen) * 8 - 4
    g = torch.rand(nnz, device=dev, generator=gen) * 2 - 1
    pbuf, dbuf = torch.empty_like(x), torch.empty_like(x)
    stream = torch.cuda.current_stream(dev).cuda_stream
    scale = 0.25

    stats, reps = cb.stats, args.reps

    eng = api.Engine(0)
    eng.set_matrix_csr_device(M, K, nnz, crow.data_ptr(), col.data_ptr(), val.data_ptr())
    e_fwd = lambda: eng.row_softmax_device(scale, x.data_ptr(), pbuf.data_ptr(), stream)
    e_bwd = lambda: eng.row_softmax_backward_device(scale, pbuf.data_ptr(), g.data_ptr(), dbuf.data_ptr(), stream)
    e_fwd(); e_bwd(); torch.cuda.synchronize()   # (the first call builds the tables)
    rec = {"matrix": args.matrix, "M": M, "K": K, "nnz": int(nnz), "rounds": args.rounds, "reps": args.reps,
           "softmax_long_rows": eng.get_stat("softmax_long_rows")}
    rec["kernel"] = eng.last_kernel()
    if args.kernels_only:
        rec["forward"] = stats([cb.timed(e_fwd, reps) for _ in range(args.rounds)])
        rec["backward"] = stats([cb.timed(e_bwd, reps) for _ in range(args.rounds)])
        cb.emit(rec, "")
        return

    rows = torch.repeat_interleave(torch.arange(M, device=dev), (crow[1:] - crow[:-1]).long())   # outside every timed region

    def compose(xv):
        s = xv * scale
        m = torch.full((M,), float("-inf"), device=dev).scatter_reduce(0, rows, s, "amax", include_self=True)
        t = torch.exp(s - m[rows])
        z = torch.zeros(M, device=dev).index_add_(0, rows, t)
        return t / z[rows]

    def b_fwd():
        with torch.no_grad():
            compose(x)

    xg = x.clone().requires_grad_()
    held = {}

    def b_fwd_graph():
        xg.grad = None
        held["p"] = compose(xg)

    def b_bwd():
        xg.grad = None   # (no accumulation into an earlier gradient: that would be one more nnz-sized pass on the baseline's side)
        held["p"].backward(g, retain_graph=True)

    b_fwd(); b_fwd_graph(); b_bwd(); torch.cuda.synchronize()
    want = held["p"].detach()
    rec["max_abs_difference_from_composition"] = float((pbuf - want).abs().max())
    ef, eb, bf, bb = [], [], [], []
    for _ in range(args.rounds):   # alternating rounds
        ef.append(cb.timed(e_fwd, reps)); bf.append(cb.timed(b_fwd, reps)); eb.append(cb.timed(e_bwd, reps)); bb.append(cb.timed(b_bwd, reps))
    for name, e, b, nbytes in (("forward", ef, bf, 8 * nnz + 4 * (M + 1)), ("backward", eb, bb, 12 * nnz + 4 * (M + 1))):
        r = stats(e)
        r["bytes"] = nbytes
        r["fraction_of_8TBps"] = nbytes / (r["median_us"] * 1e-6) / 8e12
        r["baseline"] = stats(b)
        r["ratio"] = r["baseline"]["median_us"] / r["median_us"]
        r["faster_by_more_than_the_spread"] = bool(min(b) > max(e))
        rec[name] = r
    held.clear()
    del xg, want, rows

    for d in [int(t) for t in args.steps.split(",") if t]:
        A = torch.sparse_csr_tensor(crow, col, val, size=(M, K))
        Q, Kk, V = (((torch.rand((n, d), device=dev, generator=gen) * 2 - 1) * 0.5).requires_grad_() for n in (M, K, K))
        G = torch.rand((M, d), device=dev, generator=gen) * 2 - 1
        rws = torch.repeat_interleave(torch.arange(M, device=dev), (crow[1:] - crow[:-1]).long())
        sc = 1.0 / d ** 0.5

        def clear():
            for t in (Q, Kk, V):
                t.grad = None

        def step_engine():
            clear()
            torch_op.sparse_attention(A, Q, Kk, V).backward(G)

        def step_composed():
            clear()
            S = torch_op.sddmm(A, Q, Kk)
            s = S.values() * sc
            m = torch.full((M,), float("-inf"), device=dev).scatter_reduce(0, rws, s.detach(), "amax", include_self=True)
            t = torch.exp(s - m[rws])
            z = torch.zeros(M, device=dev).index_add_(0, rws, t)
            P = torch.sparse_csr_tensor(crow, col, t / z[rws], size=(M, K))
            torch_op.spmm(P, V).backward(G)

        torch_op.clear_cache()
        step_engine(); step_composed(); torch.cuda.synchronize()
        se, sb = [], []
        for _ in range(args.rounds):
            se.append(cb.timed(step_engine, reps)); sb.append(cb.timed(step_composed, reps))
        rec["step_d%d" % d] = {"engine": stats(se), "composed": stats(sb), "ratio": statistics.median(sb) / statistics.median(se)}
        torch_op.clear_cache()
        del A, Q, Kk, V, G, rws
    cb.emit(rec, args.out)


if __name__ == "__main__":
    main()
