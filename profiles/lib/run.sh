#!/bin/bash
# Measurements of the library-type sweep.  PARENT: a checkout of the parent commit with its library built (only c needs it); OUT: where
# the lines go.  Every GPU step has a time limit of its own and the steps are chained: the first that fails ends the script.
#   bash profiles/lib/run.sh PARENT OUT [a|c ...]
set -o pipefail
PARENT=${1:?parent tree}; OUT=${2:?output directory}; shift 2
WHAT=${*:-a c}
HERE=$(cd "$(dirname "$0")/../.." && pwd)
mkdir -p "$OUT"
for w in $WHAT; do
  case $w in
  a)  # (a) qm_lib_add alone, (b) qm_eqc_add_lib under IU / ISF beside qm_eqc_add, (c) the byte floor: one process, alternating
    timeout -k 10 400 python "$HERE/profiles/lib/measure_lib.py" | tail -1 | tee "$OUT/a_sweep_and_fold.json" || exit 1 ;;
  c)  # the default path launches nothing of this: plain bench.py, parent and branch in turn
    for i in 1 2 3; do
      (cd "$PARENT" && timeout -k 10 400 python bench.py --gpus 1 --steps 8 --warmup 2 | tail -1 | tee -a "$OUT/c_bench_parent.jsonl") &&
      (cd "$HERE" && timeout -k 10 400 python bench.py --gpus 1 --steps 8 --warmup 2 | tail -1 | tee -a "$OUT/c_bench_branch.jsonl") || exit 1
    done ;;
  esac
done
