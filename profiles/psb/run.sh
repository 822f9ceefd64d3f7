#!/bin/bash
# Measurements of the positional bias kernels.  PARENT: a checkout of the parent commit with its library built (c and d need it);
# OUT: where the lines go.  Every GPU step has a time limit of its own and the steps are chained: the first that fails ends the script.
#   bash profiles/psb/run.sh PARENT OUT [ab|c|d ...]
set -o pipefail
PARENT=${1:?parent tree}; OUT=${2:?output directory}; shift 2
WHAT=${*:-ab c d}
HERE=$(cd "$(dirname "$0")/../.." && pwd)
mkdir -p "$OUT"
for w in $WHAT; do
  case $w in
  ab)  # the observed sweep beside qm_fld_add, qm_gcb_add and qm_sqb_add, qm_psb_expect, and the two effective-length walks in turn
    timeout -k 10 600 python "$HERE/profiles/psb/measure_psb.py" > "$OUT/ab_measure.log" 2>&1 || { tail -20 "$OUT/ab_measure.log"; exit 1; }
    tail -1 "$OUT/ab_measure.log" | tee "$OUT/ab_measure.json" ;;
  c)  # the parent's qm_sqb_eff_lens in the same visit: the refactor left the sequence walk where it was
    (cd "$PARENT" && timeout -k 10 600 python profiles/sqb/measure_sqb.py > "$OUT/c_parent_measure_sqb.log" 2>&1) || { tail -20 "$OUT/c_parent_measure_sqb.log"; exit 1; }
    tail -1 "$OUT/c_parent_measure_sqb.log" | tee "$OUT/c_parent_measure_sqb.json" ;;
  d)  # the default path is untouched: plain bench.py, parent and branch in turn
    for i in 1 2 3; do
      (cd "$PARENT" && timeout -k 10 500 python bench.py --gpus 1 --steps 8 --warmup 2 | tail -1 | tee -a "$OUT/d_bench_parent.jsonl") &&
      (cd "$HERE" && timeout -k 10 500 python bench.py --gpus 1 --steps 8 --warmup 2 | tail -1 | tee -a "$OUT/d_bench_branch.jsonl") || exit 1
    done ;;
  esac
done
