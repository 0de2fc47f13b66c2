"""Is the device code of two trees the same?  For a refactor that must leave the kernels alone -- of the host side (the entry points'
frame, profiles/entry_frame_device_code.txt) or of the device side itself (code moved into shared __device__ helpers,
profiles/online_softmax_device_code.txt): compiles translation units of both trees to gfx950 assembly with the flags of
sextans_amd/build.py (no GPU needed) and compares them kernel by kernel:

    git worktree add --detach ../parent HEAD~1
    python tools/device_code_diff.py ../parent . > profiles/entry_frame_device_code.txt
    python tools/device_code_diff.py ../parent . sextans_amd/csrc/engine_gat.hip      # chosen units only: a device-side change is tried per unit
    python tools/device_code_diff.py --rename '(Li\d+)EfEEEE' '\1EEEEE' ../parent . sextans_amd/csrc/engine_edge.hip
                                       # a template gained a defaulted argument: the second tree's symbols are renamed (a regular expression and
                                       # its replacement, applied to the whole assembly text) before they are matched with the first tree's

Without units: every sextans_amd/csrc/*.hip of the second tree that includes pattern_launch.h or one of the family launch headers over it
(edge_multi_launch.h, edge_op_launch.h, edge_launch.h, vector_attention_launch.h, edge_softagg_launch.h, gated_launch.h).  Either kind of
change may reorder template instantiation, so the functions are compared per symbol, not in file order, after the function's index is taken
out of its local labels (.LBB<k>_<n>, .Lfunc_end<k>).  What is compared per symbol: the instructions, the kernel descriptor, the
resource figures and the code-object metadata entry.  Exit status 1 when anything differs."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, ".")
from sextans_amd import build as b

CSRC = os.path.join("sextans_amd", "csrc")
INDEX = re.compile(r"(\.L|\b)(BB|func_begin|func_end|tmp)\d+")   # .LBB12_3 -> .LBB_3; BB12_3 in a comment likewise


def assembly(tree, unit):
    tree = os.path.abspath(tree)
    flags = [f.replace(b.ROOT, tree) for f in b.FLAGS]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        r = subprocess.run([b.hipcc()] + flags + ["--cuda-device-only", "-S", "-o", out, os.path.join(tree, unit)], capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit(f"{tree}: {unit} did not compile:\n{r.stderr[-3000:]}")
        return open(out).read()


def functions(text):
    """symbol -> its normalised text: from its .section line to the end of the info comment that follows its .size"""
    lines = text.split("\n")
    out, rest, i = {}, [], 0
    starts = []
    for k, line in enumerate(lines):
        m = re.match(r"\t\.type\t(\S+),@function", line)
        if m:
            s = k
            while s > 0 and not re.match(r"\t\.(section|text)\b", lines[s]):
                s -= 1
            starts.append((s, m.group(1)))
    for n, (s, sym) in enumerate(starts):
        limit = starts[n + 1][0] if n + 1 < len(starts) else len(lines)
        e = s
        while e < limit and not lines[e].startswith("\t.section\t.AMDGPU.csdata"):
            e += 1
        e += 1
        while e < limit and lines[e].startswith(";"):
            e += 1
        rest += lines[i:s]
        out[sym] = INDEX.sub(r"\1\2", "\n".join(lines[s:e]))
        i = e
    rest += lines[i:]
    return out, rest


def metadata(rest):
    """kernel symbol -> its entry under amdhsa.kernels"""
    entries, inside = [], False
    for line in rest:
        if line.startswith("amdhsa.kernels:"):
            inside = True
        elif inside and line.startswith("  - "):
            entries.append([line])
        elif inside and line.startswith("    "):
            entries[-1].append(line)
        else:
            inside = False
    return {next(l.split()[-1] for l in e if l.strip().startswith(".name:")): "\n".join(e) for e in entries}


RENAME = None   # (compiled pattern, replacement) for the second tree's assembly: --rename


def compare(parent, branch, unit):
    with ThreadPoolExecutor(2) as pool:
        a, c = pool.map(lambda t: assembly(t, unit), (parent, branch))
    if RENAME:
        c = RENAME[0].sub(RENAME[1], c)
    (fa, ra), (fc, rc) = functions(a), functions(c)
    ma, mc = metadata(ra), metadata(rc)
    only_a, only_c = sorted(set(fa) - set(fc)), sorted(set(fc) - set(fa))
    differing = sorted(s for s in set(fa) & set(fc) if fa[s] != fc[s] or ma.get(s) != mc.get(s))
    return len(set(fa) & set(fc)), differing, only_a, only_c


def main():
    global RENAME
    argv = sys.argv[1:]
    if argv and argv[0] == "--rename":
        RENAME, argv = (re.compile(argv[1]), argv[2]), argv[3:]
    parent, branch, units = argv[0], argv[1], argv[2:]
    if not units:
        for f in sorted(os.listdir(os.path.join(branch, CSRC))):
            if f.endswith(".hip") and re.search(r'#include "(pattern|edge_multi|edge_op|edge|vector_attention|edge_softagg|gated)_launch\.h"',
                                                open(os.path.join(branch, CSRC, f)).read()):
                units.append(os.path.join(CSRC, f))
    bad = 0
    print("# unit: functions compared, differing, only in the first tree, only in the second")
    with ThreadPoolExecutor(max(1, min(8, (os.cpu_count() or 2) // 2))) as pool:
        for unit, (n, differing, only_a, only_c) in zip(units, pool.map(lambda u: compare(parent, branch, u), units)):
            print(f"{unit}: {n} compared, {len(differing)} differing, {len(only_a)} only in the first, {len(only_c)} only in the second")
            for tag, syms in (("differs", differing), ("only in the first", only_a), ("only in the second", only_c)):
                for s in syms:
                    print(f"    {tag}: {s}")
            bad += len(differing) + len(only_a) + len(only_c)
    print(f"# total: {bad} differing or unmatched")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
