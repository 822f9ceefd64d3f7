#!/bin/bash
# Measurements (a)-(c) of the fragment-length histogram.  PARENT: a checkout of the parent commit with its library built (only (c)
# needs it); OUT: where the lines go.  Every GPU step has a time limit of its own and the steps are chained: the first that fails ends
# the script.
#   bash profiles/fld/run.sh PARENT OUT [a|b|c ...]
set -o pipefail
PARENT=${1:?parent tree}; OUT=${2:?output directory}; shift 2
WHAT=${*:-a b c}
HERE=$(cd "$(dirname "$0")/../.." && pwd)
mkdir -p "$OUT"
FQ=${QMAP_BENCH_E2E_DIR:-/tmp}/fld_$$
for w in $WHAT; do
  case $w in
  a)  # the fold at the default grid and under caps of 256 / 1 024 / 4 096 workgroups, its byte floor, qm_eqc_add's steady fold beside it
    timeout -k 10 400 python "$HERE/profiles/fld/measure_fld.py" | tail -1 | tee "$OUT/a_fold.json" || exit 1 ;;
  b)  # FASTQ -> classes with and without the histogram, same files, in turn (profiles/eq_classes/measure_stream.py writes the files)
    timeout -k 10 300 python "$HERE/profiles/eq_classes/measure_stream.py" --mode hits --fq1 "${FQ}_1.fq" --fq2 "${FQ}_2.fq" --write 10000000 | tail -1 > "$OUT/b_warm.json" || exit 1
    for i in 1 2 3; do
      timeout -k 10 200 python "$HERE/profiles/fld/measure_stream.py" --fq1 "${FQ}_1.fq" --fq2 "${FQ}_2.fq" | tail -1 | tee -a "$OUT/b_classes.jsonl" &&
      timeout -k 10 200 python "$HERE/profiles/fld/measure_stream.py" --fld --fq1 "${FQ}_1.fq" --fq2 "${FQ}_2.fq" | tail -1 | tee -a "$OUT/b_classes_fld.jsonl" || { rm -f "${FQ}"_?.fq; exit 1; }
    done
    rm -f "${FQ}"_?.fq ;;
  c)  # the default path is untouched: plain bench.py, parent and branch in turn
    for i in 1 2 3; do
      (cd "$PARENT" && timeout -k 10 400 python bench.py --gpus 1 --steps 8 --warmup 2 | tail -1 | tee -a "$OUT/c_bench_parent.jsonl") &&
      (cd "$HERE" && timeout -k 10 400 python bench.py --gpus 1 --steps 8 --warmup 2 | tail -1 | tee -a "$OUT/c_bench_branch.jsonl") || exit 1
    done ;;
  esac
done
