#!/bin/bash
# Parent and branch side by side in one GPU visit, alternating.  PARENT: a checkout of the parent commit with its library built; OUT: where
# the lines go (one JSON line per run, appended in the order the runs were made).  Every GPU step has a time limit of its own and the steps
# are chained: the first that fails ends the script.
#   bash profiles/est_objects/run.sh PARENT OUT [bench|objects|fld|lib|gcb|eqc|fold|api ...]
# ROUNDS (default 3): turns of every object's measurement; BENCH_ROUNDS (default 2): turns of parent, branch, branch, parent.
#   python profiles/est_objects/compare.py OUT > OUT/side_by_side.txt
set -o pipefail
PARENT=${1:?parent tree}; OUT=${2:?output directory}; shift 2
WHAT=${*:-bench objects fold api}
WHAT=${WHAT//objects/fld lib eqc gcb}
ROUNDS=${ROUNDS:-3}; BENCH_ROUNDS=${BENCH_ROUNDS:-2}
HERE=$(cd "$(dirname "$0")/../.." && pwd)
mkdir -p "$OUT"
bench() { (cd "$2" && timeout -k 10 420 python bench.py --gpus 1 --steps 8 --warmup 2 | tail -1 | tee -a "$OUT/bench_$1.jsonl"); }
meas() { timeout -k 10 300 python "$2/profiles/$3" | tail -1 | tee -a "$OUT/$4_$1.jsonl"; }
for w in $WHAT; do
  case $w in
  bench)    # the default path launches nothing of the estimation objects: plain bench.py
    for i in $(seq "$BENCH_ROUNDS"); do
      bench parent "$PARENT" && bench branch "$HERE" && bench branch "$HERE" && bench parent "$PARENT" || exit 1
    done ;;
  # the objects, per fold / per sweep, by HIP events on the stream (`objects`: all four)
  fld) for i in $(seq "$ROUNDS"); do meas parent "$PARENT" fld/measure_fld.py fld && meas branch "$HERE" fld/measure_fld.py fld || exit 1; done ;;
  lib) for i in $(seq "$ROUNDS"); do meas branch "$HERE" lib/measure_lib.py lib && meas parent "$PARENT" lib/measure_lib.py lib || exit 1; done ;;
  eqc) for i in $(seq "$ROUNDS"); do meas parent "$PARENT" eq_classes/measure_fold.py fold && meas branch "$HERE" eq_classes/measure_fold.py fold || exit 1; done ;;
  gcb)      # (the order turned every round: the rank structure's build is timed once per process, right after it starts)
    for i in $(seq "$ROUNDS"); do
      if [ $((i % 2)) = 1 ]; then meas branch "$HERE" gcb/measure_gcb.py gcb && meas parent "$PARENT" gcb/measure_gcb.py gcb || exit 1
      else meas parent "$PARENT" gcb/measure_gcb.py gcb && meas branch "$HERE" gcb/measure_gcb.py gcb || exit 1; fi
    done ;;
  fold)     # the equivalence-class fold again, the order turned every pair: its time differs more between processes than within one
    for i in 1 2 3; do
      meas branch "$HERE" eq_classes/measure_fold.py fold && meas parent "$PARENT" eq_classes/measure_fold.py fold &&
      meas parent "$PARENT" eq_classes/measure_fold.py fold && meas branch "$HERE" eq_classes/measure_fold.py fold || exit 1
    done ;;
  api)      # HIP API calls of 1 and of 11 folds / sweeps: runs of their own under a HIP trace, no counters (api_calls.py prints the table)
    mkdir -p "$OUT/api"
    for what in fld lib gcb; do for n in 1 11; do for t in parent branch; do
      root=$HERE; [ $t = parent ] && root=$PARENT
      timeout -k 10 200 rocprofv3 --hip-trace --stats -d "$OUT/api/${what}_${n}_$t" -o t --output-format csv -- \
        python "$HERE/profiles/est_objects/api_calls.py" run "$root" $what $n > "$OUT/api/${what}_${n}_$t.log" 2>&1 || exit 1
    done; done; done
    python "$HERE/profiles/est_objects/api_calls.py" table "$OUT/api" > "$OUT/hip_api_calls.txt" ;;
  esac
done
