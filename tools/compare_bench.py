"""The measurement protocol of the fused-op comparison tools (tools/*_bench.py), defined once: DESIGN 4.10 / 4.12 cite it.

A tool times its op ("fused", or the op's own name) against what a user can write without it, on the same commit, in the same process
and on the same tensors, on one GPU.  Per case: the forward alone (no autograd graph) and forward + backward, each side timed between HIP
events over --rounds rounds of `reps` calls, the sides in ALTERNATING rounds after one untimed warm-up step per side (engine, A^T, plans
and tables are built there); reps is chosen per record so that a round of the slowest side lasts about --round-ms.
"spread" = (max - min) / median of a side's rounds.  "ratio" = other median / subject median (> 1: the subject is faster).  "verdict": a
side's name when its slowest round beats the other's fastest -- a difference larger than the spread between repeats -- else "undecided".
"peak_bytes": torch.cuda.max_memory_allocated over one forward + backward step of a side, above what was allocated before it.  A side
that cannot be allocated is recorded as such by the tool, and the others are timed without it.
--tag NAME is written into every record and says which build it timed; --out FILE gets one JSON line per record, appended.

Matrices (load_matrix): "config4" = gen_csr_device(4 M, 4 M, Poisson(40)), "fem" = gen_fem3d_device(110, 110, 110, 3) (3.99 M rows,
318 M non-zeros), "powerlaw" = gen_powerlaw_device(1 M, 1 M, 6, 1.2, 400 000), "small" = a 200 k-row config-4 for trying a tool out.

These are functions the tools call; a tool keeps its operands, its sides, its record's own fields and its loops.  Importing this module
needs neither torch nor a GPU.

    python tools/compare_bench.py --diff A.jsonl B.jsonl     key trees and non-timing values of two runs, record by record"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MATRICES = ("config4", "fem", "powerlaw", "small")
PASSES = ("forward", "forward_backward")


def add_protocol_args(ap, tag=True):
    """--matrix, --rounds, --round-ms, --max-reps, --out, and --tag for the tools whose records carry one"""
    ap.add_argument("--matrix", choices=list(MATRICES), default="small")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--round-ms", type=float, default=200.0)
    ap.add_argument("--max-reps", type=int, default=8)
    if tag:
        ap.add_argument("--tag", default="", help="written into every record as \"tag\" (names the build that was timed)")
    ap.add_argument("--out", default="")


def load_matrix(name):
    """-> (A, crow, col, val, M, K, nnz): the generated matrix as int32 / fp32 torch tensors on GPU 0 and the sparse_csr tensor on them"""
    import torch
    from sextans_amd import api
    dev = torch.device("cuda", 0)
    if name == "fem":
        M = K = 110 ** 3 * 3
        p, i, v, nnz = api.gen_fem3d_device(0, 110, 110, 110, 3, 3)
    elif name == "powerlaw":
        M = K = 1_000_000
        p, i, v, nnz = api.gen_powerlaw_device(0, M, K, 6, 120, 400_000, 7)
    else:
        M = K = 4_000_000 if name == "config4" else 200_000
        p, i, v, nnz = api.gen_csr_device(0, M, K, 40.0, 4)
    nnz = int(nnz)
    crow = torch.empty(M + 1, dtype=torch.int32, device=dev); col = torch.empty(nnz, dtype=torch.int32, device=dev)
    val = torch.empty(nnz, dtype=torch.float32, device=dev)
    for dst, src, n in ((crow, p, (M + 1) * 4), (col, i, nnz * 4), (val, v, nnz * 4)):
        api.device_copy(0, dst.data_ptr(), src, n)
        api.device_free(0, src)
    return torch.sparse_csr_tensor(crow, col, val, size=(M, K)), crow, col, val, M, K, nnz


def timed(fn, reps):
    import torch
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


def verdict(subject_ts, other_ts, subject_name="fused", other_name="composition"):
    """-> (other median / subject median, the side whose slowest round beats the other's fastest, else "undecided")"""
    ratio = statistics.median(other_ts) / statistics.median(subject_ts)
    return ratio, subject_name if max(subject_ts) < min(other_ts) else other_name if max(other_ts) < min(subject_ts) else "undecided"


def two_sided(subject_ts, other_ts, subject_name="fused", other_name="composition"):
    """the block of a comparison that carries both sides: their statistics, "ratio", "verdict\""""
    r = {subject_name: stats(subject_ts), other_name: stats(other_ts)}
    r["ratio"], r["verdict"] = verdict(subject_ts, other_ts, subject_name, other_name)
    return r


def pass_block(ts):
    """the block of one pass of "fused" against "composition"; the fused side's statistics alone where no composition was timed"""
    return two_sided(ts["fused"], ts["composition"]) if "composition" in ts else {"fused": stats(ts["fused"])}


def baseline_block(subject_ts, other_ts, subject_name="fused", other_name="composition"):
    """the block of one baseline among several: ITS statistics, with "ratio" and "verdict" against the subject (whose block stands beside)"""
    r = stats(other_ts)
    r["ratio"], r["verdict"] = verdict(subject_ts, other_ts, subject_name, other_name)
    return r


def choose_reps(once_us, round_ms, max_reps):
    """calls per round, so that a round lasts about round_ms: at least 1, at most max_reps"""
    return int(max(1, min(max_reps, round_ms * 1e3 / once_us)))


def peak_of_step(step, leaves):
    """One untimed step (the warm-up), the gradients of `leaves` cleared, then the peak of a second step above what was allocated before it."""
    import torch
    dev = torch.device("cuda", 0)
    step()
    for t in leaves:
        t.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    step()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated(dev) - base)


def warm_up_peaks(step, leaves, sides, may_fail=()):
    """Warm-up and peak bytes, side by side: yields (side, peak_of_step of step(side)) in the order given, and (side, None) for a side of
    `may_fail` that ran out of memory (gradients cleared, cache emptied); on any other side the error propagates.  What a lost side is
    recorded as, and what is tidied between two sides, is the caller's loop body."""
    import torch
    for side in sides:
        try:
            nbytes = peak_of_step(lambda: step(side), leaves)
        except torch.OutOfMemoryError:
            if side not in may_fail:
                raise
            for t in leaves:
                t.grad = None
            torch.cuda.empty_cache()
            nbytes = None
        yield side, nbytes


def slowest_once(fn, sides):
    """the one timing call per side that sizes reps: the slowest side's time"""
    return max(timed(lambda: fn(s), 1) for s in sides)


def slowest_once_dropping(fn, sides, drop="composition"):
    """slowest_once -> (time, False); where a call runs out of memory (the step fitted once, or the other way round), `drop` leaves
    `sides`, in place, and the rest is timed again -> (time, True)"""
    import torch
    try:
        return slowest_once(fn, sides), False
    except torch.OutOfMemoryError:
        torch.cuda.empty_cache()
        sides.remove(drop)
        return slowest_once(fn, sides), True


def rounds_at(fn, sides, once_us, args):
    """args.rounds alternating rounds of `sides` in the order given, at the reps once_us asks for -> ({side: times}, reps)"""
    reps = choose_reps(once_us, args.round_ms, args.max_reps)
    ts = {s: [] for s in sides}
    for _ in range(args.rounds):   # alternating rounds
        for s in ts:
            ts[s].append(timed(lambda: fn(s), reps))
    return ts, reps


def alternating_rounds(fn, sides, args, also=()):
    """`sides` size reps (the slowest of them); `also`, timed for information, takes its turn after them in every round"""
    return rounds_at(fn, list(sides) + list(also), slowest_once(fn, sides), args)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as fh:
            fh.write(line + "\n")


def read_records(out, matrix):
    with open(out) as fh:
        return [r for r in map(json.loads, fh) if r["matrix"] == matrix]


def summary_line(recs, matrix, title, label, block, missing="composition: out of memory"):
    """Per workload: does the subject beat the other side by more than the spread between repeats?  One line, "label verdict xratio" per
    record; block(r) is the record's block that holds the verdict, `missing` (a text, or a function of the record) stands in where it
    holds none."""
    parts = []
    for r in recs:
        b = block(r)
        parts.append("%s %s" % (label(r), "%s x%.2f" % (b["verdict"], b["ratio"]) if isinstance(b, dict) and "verdict" in b
                                else missing(r) if callable(missing) else missing))
    print("%s %s: %s" % (matrix, title, "; ".join(parts)))


TIMING_KEYS = ("median_us", "min_us", "max_us", "spread", "ratio", "verdict", "reps", "fraction_of_8TBps", "faster_by_more_than_the_spread")


def _walk(x, path=""):
    """(path, value) of every leaf, in the record's own order; a time or what follows from times (TIMING_KEYS) counts as a key without a
    value.  Peak bytes are compared: one step of the same code on the same tensors allocates the same."""
    if isinstance(x, dict):
        for k, v in x.items():
            if k in TIMING_KEYS:
                yield path + "/" + k, None
            else:
                yield from _walk(v, path + "/" + k)
    else:
        yield path, x


def diff(path_a, path_b):
    """prints where two runs' records differ in key tree, key order or a value that is no measurement -> the number of such records"""
    with open(path_a) as fa, open(path_b) as fb:
        a, b = [json.loads(x) for x in fa], [json.loads(x) for x in fb]
    bad = abs(len(a) - len(b))
    if bad:
        print("records: %d against %d" % (len(a), len(b)))
    for n, (ra, rb) in enumerate(zip(a, b)):
        la, lb = list(_walk(ra)), list(_walk(rb))
        if la != lb:
            bad += 1
            for x in la:
                if x not in lb:
                    print("record %d, first only: %s = %r" % (n, x[0], x[1]))
            for x in lb:
                if x not in la:
                    print("record %d, second only: %s = %r" % (n, x[0], x[1]))
            if sorted(map(repr, la)) == sorted(map(repr, lb)):
                print("record %d: same keys and values, another key order" % n)
    print("%s %s: %d records, %d differ" % (path_a, path_b, min(len(a), len(b)), bad))
    return bad


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--diff":
        sys.exit(1 if diff(sys.argv[2], sys.argv[3]) else 0)
    sys.exit(__doc__)
