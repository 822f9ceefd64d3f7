#!/bin/bash
# Measurements (a)-(d) of the variational Bayes EM.  PARENT: a checkout of the parent commit with its library built ((c) and (d) need
# it); OUT: where the lines go.  Every GPU step has a time limit of its own and the steps are chained: the first that fails ends the
# script.
#   bash profiles/vb/run.sh PARENT OUT [ab|c|d ...]
set -o pipefail
PARENT=${1:?parent tree}; OUT=${2:?output directory}; shift 2
WHAT=${*:-ab c d}
HERE=$(cd "$(dirname "$0")/../.." && pwd)
mkdir -p "$OUT"
for w in $WHAT; do
  case $w in
  ab)   # time per iteration of both methods in one process beside the byte floor; convergence at the defaults
    timeout -k 10 500 python "$HERE/profiles/vb/measure_vb.py" | tail -1 | tee "$OUT/ab_vb.json" || exit 1 ;;
  c)    # the EM is unchanged: the EM's own measurement, parent and branch in turn (part (b) of its line is what is compared)
    for i in 1 2 3; do
      (cd "$PARENT" && timeout -k 10 500 python profiles/quant/measure_quant.py | tail -1 | tee -a "$OUT/c_quant_parent.jsonl") &&
      (cd "$HERE" && timeout -k 10 500 python profiles/quant/measure_quant.py | tail -1 | tee -a "$OUT/c_quant_branch.jsonl") || exit 1
    done ;;
  d)    # the default path launches nothing new: plain bench.py, parent and branch in turn
    for i in 1 2 3; do
      (cd "$PARENT" && timeout -k 10 400 python bench.py --gpus 1 --steps 8 --warmup 2 | tail -1 | tee -a "$OUT/d_bench_parent.jsonl") &&
      (cd "$HERE" && timeout -k 10 400 python bench.py --gpus 1 --steps 8 --warmup 2 | tail -1 | tee -a "$OUT/d_bench_branch.jsonl") || exit 1
    done ;;
  esac
done
