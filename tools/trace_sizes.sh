#!/bin/bash
# kernel traces of single proofs at the BASELINE sizes (run from the repo root on a machine with the GPU): $OUT/kt<n>/ (OUT defaults to bench_out)
set -u
export TMPDIR=/tmp
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
for n in "$@"; do
  rm -rf $OUT/kt$n
  rocprofv3 --kernel-trace --output-format csv -d $OUT/kt$n -- python3 bench.py --full --log-domain $n --steps 6 --warmup 2 --no-cpu-baseline --no-by-config --no-end-to-end --no-reconstruct --batch 1 --in-flight 1 --batch-extra 0 --sequential-extra 0 > $OUT/kt$n.json 2> $OUT/kt$n.err
  python3 tools/proof_timeline.py $OUT/kt$n 12 > $OUT/timeline$n.txt 2>&1
  # keep only the per-proof text and the bench line (the raw trace is large)
  rm -rf $OUT/kt$n
done
