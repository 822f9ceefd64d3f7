#!/bin/bash
# Measurements of the sequence-specific bias kernels.  PARENT: a checkout of the parent commit with its library built (only d needs
# it); OUT: where the lines go.  Every GPU step has a time limit of its own and the steps are chained: the first that fails ends the script.
#   bash profiles/sqb/run.sh PARENT OUT [abc|d ...]
set -o pipefail
PARENT=${1:?parent tree}; OUT=${2:?output directory}; shift 2
WHAT=${*:-abc d}
HERE=$(cd "$(dirname "$0")/../.." && pwd)
mkdir -p "$OUT"
for w in $WHAT; do
  case $w in
  abc)  # (a) the observed sweep beside qm_gcb_add and qm_fld_add, (b) qm_sqb_expect, (c) qm_sqb_eff_lens on the config-2 index
    timeout -k 10 600 python "$HERE/profiles/sqb/measure_sqb.py" > "$OUT/abc_measure.log" 2>&1 || { tail -20 "$OUT/abc_measure.log"; exit 1; }
    tail -1 "$OUT/abc_measure.log" | tee "$OUT/abc_measure.json" ;;
  d)  # the default path is untouched: plain bench.py, parent and branch in turn
    for i in 1 2 3; do
      (cd "$PARENT" && timeout -k 10 500 python bench.py --gpus 1 --steps 8 --warmup 2 | tail -1 | tee -a "$OUT/d_bench_parent.jsonl") &&
      (cd "$HERE" && timeout -k 10 500 python bench.py --gpus 1 --steps 8 --warmup 2 | tail -1 | tee -a "$OUT/d_bench_branch.jsonl") || exit 1
    done ;;
  esac
done
