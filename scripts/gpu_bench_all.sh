#!/bin/bash
# Full bench lines (every leg) for C2 (default), C3, C4, C5 on one GPU -> $OUT/bench_c<config>.log
cd "$(dirname "$0")/.." || exit 1; OUT=${OUT:-bench_out}; mkdir -p "$OUT"; export TMPDIR=/tmp
for c in 2 3 4 5; do
  timeout -k 10 400 python3 bench.py --full --config $c > "$OUT/bench_c$c.log" 2>&1 || exit $?
done
