#!/bin/bash
# tools/evidence_r06.sh <out> -- the round-6 evidence run on one MI355X box; every record goes under <out> (relative to the repo root).
#  1. the bench line as the driver runs it (two stdout lines since round 6: {"also": ...} then the headline object) + the forced
#     1-rank distributed forms (sextans_dist_prepare + sextans_dist_spmm / _rm over a real 1-rank RCCL communicator);
#  2. kernel-trace statistics PER WORKLOAD (one rocprofv3 pass for the headline and one per `also` entry);
#  3. PMC passes of the headline (tools/prof.sh r06 -> config-4 traffic).
cd "$(dirname "$0")/.."
REPO=$(pwd)
OUT=${1:?usage: tools/evidence_r06.sh <output folder>}
export TMPDIR=/tmp
mkdir -p $OUT/r06_kernel_stats
python bench.py --steps 20 --warmup 5 --full > $OUT/r06_bench_stdout.txt 2> $OUT/r06_bench_stderr.txt
tail -1 $OUT/r06_bench_stdout.txt > $OUT/r06_bench_final.json
SEXTANS_BENCH_FORCE_DIST=1 python bench.py --steps 20 --warmup 5 --full --no-also --no-cpu-baseline 2>/dev/null | tail -1 > $OUT/r06_bench_forced_dist_colmajor.json
SEXTANS_BENCH_FORCE_DIST=1 python bench.py --steps 20 --warmup 5 --full --no-also --no-cpu-baseline --rowmajor 2>/dev/null | tail -1 > $OUT/r06_bench_forced_dist_rowmajor.json
stats() {   # stats <key> <command...>
  local key=$1; shift
  rm -rf /tmp/rp_$key
  (cd /tmp && timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/rp_$key -o s -- "$@" > $REPO/$OUT/r06_kernel_stats/$key.log 2>&1)
  find /tmp/rp_$key -name "*kernel_stats.csv" -exec cp {} $OUT/r06_kernel_stats/$key.csv \;
}
stats headline_config4 python $REPO/bench.py --steps 20 --warmup 3 --no-cpu-baseline --no-also
for KEY in $(python bench.py --only list 2>/dev/null | tail -1); do stats $KEY python $REPO/bench.py --only $KEY; done
python tools/merge_kernel_stats.py $OUT/r06_kernel_stats > $OUT/r06_bench_kernel_stats_per_workload.csv
bash tools/prof.sh r06
