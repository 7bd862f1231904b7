#!/bin/bash
# GPU box: A/B of an environment switch on bench.py, interleaved on one box.  tools/ab_env.sh <VAR> "<configs>" <out> [reps] [A B]
# (A B: the two values, 0 and 1 unless given -- e.g. POD_MI355X_LIB with two builds of the library)
set -u
var=$1; out=$3; reps=${4:-2}; va=${5:-0}; vb=${6:-1}; mkdir -p $(dirname $out); : > $out
for c in $2; do for r in $(seq $reps); do for v in "$va" "$vb"; do
  line=$(env $var=$v python bench.py --config $c --steps 150 --warmup 20 --no-cpu-baseline --no-diagnostics 2>/dev/null | grep '^{' | tail -1 | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('%.1f images/s  %.3f ms/step' % (d['value'], d['ms_per_step']))")
  echo "$c $var=$v  $line" | tee -a $out
done; done; done
