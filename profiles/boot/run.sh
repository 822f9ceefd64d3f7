#!/bin/bash
# Measurements (a)-(d) of the bootstrap replicates.  PARENT: a checkout of the parent commit with its library built (only (d) needs
# it); OUT: where the lines go.  Every GPU step has a time limit of its own and the steps are chained: the first that fails ends the script.
#   bash profiles/boot/run.sh PARENT OUT [abc|d ...]
set -o pipefail
PARENT=${1:?parent tree}; OUT=${2:?output directory}; shift 2
WHAT=${*:-abc d}
HERE=$(cd "$(dirname "$0")/../.." && pwd)
mkdir -p "$OUT"
for w in $WHAT; do
  case $w in
  abc)  # resample with and without aggregation, time per iteration per replicate beside Quant's and the byte floor, convergence
    timeout -k 10 900 python "$HERE/profiles/boot/measure_boot.py" | tee "$OUT/abc_boot.jsonl" || exit 1 ;;
  d)    # the default path is untouched: plain bench.py, parent and branch in turn
    for i in 1 2 3; do
      (cd "$PARENT" && timeout -k 10 400 python bench.py --gpus 1 --steps 8 --warmup 2 | tail -1 | tee -a "$OUT/d_bench_parent.jsonl") &&
      (cd "$HERE" && timeout -k 10 400 python bench.py --gpus 1 --steps 8 --warmup 2 | tail -1 | tee -a "$OUT/d_bench_branch.jsonl") || exit 1
    done ;;
  esac
done
