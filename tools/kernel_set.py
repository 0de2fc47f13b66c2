"""The device code of a built library, in a form two builds can be compared by (`diff -r` of two output directories):

    python tools/kernel_set.py sextans_amd/lib/libsextans_amd.so OUTDIR [NAMELESS_REGEX]

Unbundles the gfx950 code objects of the library (llvm-objdump --offloading) and writes, one line per distinct kernel name (the .kd symbols):
  names.txt   the sorted names                     counts.txt  in how many code objects the kernel appears
  res.txt     VGPR / AGPR / SGPR / LDS / scratch / spill figures from the code-object notes
  dis.txt     SHA-256 of the kernel's disassembly, instruction text only (no addresses, no encodings, no padding behind the last s_endpgm)
Used for profiles/engine_split_kernels.txt: a host-only change leaves all four files as they were.
With NAMELESS_REGEX (searched in the mangled names) two more files, for a change that RENAMES kernels without touching their code:
  multiset.txt  the matching kernels as sorted "dis-hash | res row | copies" lines, no names: equal before and after such a change
  rest.txt      every other kernel as "name copies | res row | dis-hash": a diff of two builds' files is empty
Used for profiles/pattern_pass_kernels.txt."""
import collections
import hashlib
import os
import re
import shutil
import subprocess
import sys

LLVM = os.path.dirname(shutil.which("llvm-objdump") or "/opt/rocm/llvm/bin/llvm-objdump") + "/"
lib, out = sys.argv[1], sys.argv[2]
shutil.rmtree(out, ignore_errors=True)
os.makedirs(out)
tmp = os.path.join(out, "lib.so")
shutil.copy(lib, tmp)
subprocess.run([LLVM + "llvm-objdump", "--offloading", tmp], check=True, stdout=subprocess.DEVNULL)
cos = sorted(f for f in os.listdir(out) if "gfx950" in f)
count = collections.Counter()
res = {}
dis = {}
for co in cos:
    p = os.path.join(out, co)
    sym = subprocess.run([LLVM + "llvm-readelf", "-sW", p], check=True, capture_output=True, text=True).stdout
    names = {l.split()[-1][:-3] for l in sym.splitlines() if l.strip().endswith(".kd")}
    for n in names:
        count[n] += 1
    notes = subprocess.run([LLVM + "llvm-readelf", "--notes", p], check=True, capture_output=True, text=True).stdout
    for blk in re.split(r"\n\s+- ", notes):
        m = re.search(r"\.name:\s+(\S+)", blk)
        if not m or ".vgpr_count" not in blk:
            continue
        f = {k: re.search(r"\." + k + r":\s+(\S+)", blk) for k in
             ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "max_flat_workgroup_size")}
        res.setdefault(m.group(1), set()).add(" ".join("%s=%s" % (k, v.group(1) if v else "-") for k, v in f.items()))
    d = subprocess.run([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", p], check=True, capture_output=True, text=True).stdout
    cur = None
    buf = []
    def flush():
        while buf and buf[-1] in ("", "s_nop 0", "..."):   # the padding behind a kernel depends on what follows it in .text, not on the kernel
            buf.pop()
        if cur is not None and cur in names:
            dis.setdefault(cur, set()).add(hashlib.sha256("\n".join(buf).encode()).hexdigest())
    for l in d.splitlines():
        m = re.match(r"^<?(\S+?)>?:$", l.strip()) if l.endswith(">:") else None
        if m:
            flush()
            cur, buf = m.group(1).strip("<>"), []
        else:
            buf.append(l.split("//")[0].strip())
    flush()
with open(os.path.join(out, "names.txt"), "w") as f:
    f.write("\n".join(sorted(count)) + "\n")
with open(os.path.join(out, "counts.txt"), "w") as f:
    f.write("".join("%s %d\n" % (n, count[n]) for n in sorted(count)))
with open(os.path.join(out, "res.txt"), "w") as f:
    f.write("".join("%s %s\n" % (n, " | ".join(sorted(res.get(n, ["?"])))) for n in sorted(count)))
with open(os.path.join(out, "dis.txt"), "w") as f:
    f.write("".join("%s %s\n" % (n, " ".join(sorted(dis.get(n, ["?"])))) for n in sorted(count)))
if len(sys.argv) > 3:
    row = lambda n: (" ".join(sorted(dis.get(n, ["?"]))), " | ".join(sorted(res.get(n, ["?"]))), count[n])
    match = [n for n in sorted(count) if re.search(sys.argv[3], n)]
    with open(os.path.join(out, "multiset.txt"), "w") as f:
        f.write("".join(sorted("%s | %s | %d\n" % row(n) for n in match)))
    with open(os.path.join(out, "rest.txt"), "w") as f:
        f.write("".join("%s %d | %s | %s\n" % (n, row(n)[2], row(n)[1], row(n)[0]) for n in sorted(count) if n not in match))
    print(len(match), "kernels match", sys.argv[3])
print(len(cos), "gfx950 code objects,", len(count), "distinct kernels,", sum(count.values()), "kernel copies,",
      sum(1 for n in count if n not in res), "without notes,", sum(1 for n in count if n not in dis), "without disassembly")
