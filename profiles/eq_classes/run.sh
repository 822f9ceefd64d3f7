#!/bin/bash
# Measurements (a)-(c) of the equivalence-class table.  PARENT: a checkout of the parent commit with its library built; OUT: where the
# lines go.  Every GPU step has a time limit of its own and the steps are chained: the first that fails ends the script.
#   bash profiles/eq_classes/run.sh PARENT OUT [a|k|b|c ...]
set -o pipefail
PARENT=${1:?parent tree}; OUT=${2:?output directory}; shift 2
WHAT=${*:-a k b c}
HERE=$(cd "$(dirname "$0")/../.." && pwd)
mkdir -p "$OUT"
FQ=${QMAP_BENCH_E2E_DIR:-/tmp}/eqc_$$
for w in $WHAT; do
  case $w in
  a)  # fold against download: the branch (download, fold into an empty table, steady fold, steady without aggregation; three turns), then the parent's download
    timeout -k 10 400 python "$HERE/profiles/eq_classes/measure_fold.py" | tail -1 | tee "$OUT/a_fold_branch.json" &&
    timeout -k 10 400 python "$HERE/profiles/eq_classes/measure_fold.py" --root "$PARENT" --no-fold | tail -1 | tee "$OUT/a_fetch_parent.json" || exit 1 ;;
  k)  # the fold by kernel: one warm-up fold into an empty table and one steady fold under rocprofv3
    (cd "$OUT" && timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/rocprof" -o fold -- python "$HERE/profiles/eq_classes/measure_fold.py" --once | tail -1) &&
    python - "$OUT" <<'PY' || exit 1
import csv, glob, sys
f = glob.glob(sys.argv[1] + "/rocprof/**/*kernel_stats.csv", recursive=True)
rows = [r for r in csv.DictReader(open(f[0])) if "eqc" in r["Name"]]
open(sys.argv[1] + "/a_fold_kernels.txt", "w").write("\n".join("%-60s calls %4s total %10.3f ms avg %9.3f ms" % (r["Name"][:60], r["Calls"], float(r["TotalDurationNs"]) / 1e6, float(r["AverageNs"]) / 1e6) for r in rows) + "\n")
print(open(sys.argv[1] + "/a_fold_kernels.txt").read())
PY
    rm -rf "$OUT/rocprof" || exit 1 ;;
  b)  # FASTQ -> classes (branch, no hits leave the device) against FASTQ -> hits (parent), same files, in turn
    timeout -k 10 300 python "$HERE/profiles/eq_classes/measure_stream.py" --mode hits --fq1 "${FQ}_1.fq" --fq2 "${FQ}_2.fq" --write 10000000 | tail -1 > "$OUT/b_warm.json" || exit 1
    for i in 1 2 3; do
      timeout -k 10 200 python "$HERE/profiles/eq_classes/measure_stream.py" --root "$PARENT" --mode hits --fq1 "${FQ}_1.fq" --fq2 "${FQ}_2.fq" | tail -1 | tee -a "$OUT/b_hits_parent.jsonl" &&
      timeout -k 10 200 python "$HERE/profiles/eq_classes/measure_stream.py" --mode classes --fq1 "${FQ}_1.fq" --fq2 "${FQ}_2.fq" | tail -1 | tee -a "$OUT/b_classes_branch.jsonl" || { rm -f "${FQ}"_?.fq; exit 1; }
    done
    rm -f "${FQ}"_?.fq ;;
  c)  # the default path is untouched: plain bench.py, parent and branch in turn
    for i in 1 2 3; do
      (cd "$PARENT" && timeout -k 10 400 python bench.py --gpus 1 --steps 8 --warmup 2 | tail -1 | tee -a "$OUT/c_bench_parent.jsonl") &&
      (cd "$HERE" && timeout -k 10 400 python bench.py --gpus 1 --steps 8 --warmup 2 | tail -1 | tee -a "$OUT/c_bench_branch.jsonl") || exit 1
    done ;;
  esac
done
