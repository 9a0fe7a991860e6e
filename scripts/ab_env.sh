#!/bin/bash
# same-box A/B of an environment switch of the library (TDOA_NO_...=1) against the default path
# usage: scripts/ab_env.sh TAG "VAR=1" "bench flags"   -> $OUT/r04/abe_<TAG>_<default|switch>_<n>.json
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-bench_out}; mkdir -p "$OUT"            # where the runs write (OUT=<dir> to choose)
tag=$1
mkdir -p $OUT/r04
for n in 1 2 3; do
  for mode in default switch; do
    f=$OUT/r04/abe_${tag}_${mode}_$n
    if [ $mode = switch ]; then
      env "$2" python3 bench.py --full --no-cpu-baseline --no-graph-leg --no-h2d $3 > $f.json 2> $f.err || exit 1
    else
      python3 bench.py --full --no-cpu-baseline --no-graph-leg --no-h2d $3 > $f.json 2> $f.err || exit 1
    fi
    python3 -c "import json; d=json.load(open('$f.json')); print('$tag $mode $n', d['ms_per_step'], d['roofline']['kernels_ms_per_step'])"
  done
done
