#!/bin/bash
# C4 and C5 full bench lines (no CPU leg) + kernel-trace stats of a plain run -> $OUT
cd "$(dirname "$0")/.." || exit 1; OUT=${OUT:-bench_out}; mkdir -p "$OUT"; export TMPDIR=/tmp
for c in 4 5; do
  timeout -k 10 300 python3 bench.py --full --config $c --no-cpu > "$OUT/c${c}_bench.log" 2>&1 || exit $?
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/c${c}prof" -o c$c --output-format csv -- python3 bench.py --config $c --steps 5 --warmup 2 > "$OUT/c${c}_prof.log" 2>&1 || exit $?
  find "$OUT/c${c}prof" -name "*kernel_stats.csv" -exec cp {} "$OUT/c${c}_kernel_stats.csv" \;
done
