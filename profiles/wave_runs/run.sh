#!/bin/bash
# Measurements of the headline kernels' launch geometry: one-wave workgroups and runs of neighbouring pairs per wave (qm_grid.h).
#   bash profiles/wave_runs/run.sh PARENT_LIB WG4_LIB OUT [same|sweep|bench|small|trace|pmc|sum ...]
# PARENT_LIB: libqmap_mi355.so built from the parent commit; WG4_LIB: this tree's library built with -DQM_WG_WAVES=4 (four-wave
# workgroups, the parent's shape); the tree's own library has one-wave workgroups.  QM_WAVE_RUN sets the run length at run time.
# Every GPU step has a time limit of its own and the steps are chained: the first that fails ends the script.  Counter passes are runs
# of their own (--pmc alone).  profiles/wave_runs/summarize.py turns OUT into the tables under results/.
set -o pipefail
PARENT=${1:?parent library}; WG4=${2:?library built with -DQM_WG_WAVES=4}; OUT=${3:?output directory}; shift 3
WHAT=${*:-same sweep bench small trace pmc sum}
HERE=$(cd "$(dirname "$0")/../.." && pwd)
mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
cd "$HERE" || exit 1
BENCH="python bench.py --gpus 1 --steps 10 --warmup 3"
QUIET="--no-cpu-baseline --no-other-configs --no-side-legs --no-input-variants"
# one bench line of library $2 (empty: the tree's) at QM_WAVE_RUN=$3 (empty: the default), appended to $OUT/$1.jsonl; $4..: more bench flags
line() {
  local name=$1 lib=$2 run=$3; shift 3
  env ${lib:+QM_LIB_OVERRIDE=$lib} ${run:+QM_WAVE_RUN=$run} timeout -k 10 300 $BENCH "$@" | tail -1 >> "$OUT/$name.jsonl"
}
for w in $WHAT; do
  case $w in
  same)  # the same answers: sha256 of every file bench.py --dump-outputs writes, parent and branch
    QM_LIB_OVERRIDE=$PARENT timeout -k 10 300 $BENCH --dump-outputs "$OUT/dump_parent" > "$OUT/dump_parent.log" 2>&1 &&
    timeout -k 10 300 $BENCH --dump-outputs "$OUT/dump_branch" > "$OUT/dump_branch.log" 2>&1 &&
    (cd "$OUT/dump_parent" && sha256sum *.npy) > "$OUT/dump_parent.sha256" && (cd "$OUT/dump_branch" && sha256sum *.npy) > "$OUT/dump_branch.sha256" || exit 1
    cmp "$OUT/dump_parent.sha256" "$OUT/dump_branch.sha256" && echo "dump-outputs: equal" || { echo "dump-outputs: DIFFER"; exit 1; } ;;
  sweep)  # R x waves per workgroup, the parent before and after each round
    for i in 1 2 3 4; do
      line sweep_parent "$PARENT" "" &&
      line sweep_wg1_r1 "" 1 && line sweep_wg1_r2 "" 2 && line sweep_wg1_r4 "" 4 && line sweep_wg1_r8 "" 8 &&
      line sweep_wg4_r1 "$WG4" 1 && line sweep_wg4_r2 "$WG4" 2 && line sweep_wg4_r4 "$WG4" 4 && line sweep_wg4_r8 "$WG4" 8 || exit 1
    done
    line sweep_parent "$PARENT" "" || exit 1 ;;
  bench)  # the headline: parent and branch (the tree's library, its defaults) alternating, fresh processes
    for i in 1 2 3 4 5; do line bench_parent "$PARENT" "" && line bench_branch "" "" || exit 1; done ;;
  small)  # the small-batch regime of the call surface
    for i in 1 2 3 4 5; do line small_parent "$PARENT" "" --pairs 100000 --steps 50 && line small_branch "" "" --pairs 100000 --steps 50 || exit 1; done ;;
  trace)  # per-kernel durations and the stage-A span
    for v in parent branch; do
      lib=""; [ $v = parent ] && lib=$PARENT
      env ${lib:+QM_LIB_OVERRIDE=$lib} timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/trace_$v" -o t -- $BENCH $QUIET > "$OUT/trace_$v.log" 2>&1 || { tail -5 "$OUT/trace_$v.log"; exit 1; }
    done ;;
  pmc)  # each kernel alone over the 10 M pairs (QM_SPLIT=1: one part), two counter passes each
    for v in parent branch; do
      lib=""; [ $v = parent ] && lib=$PARENT
      for kern in lean duo; do
        knob=QM_NO_DUO=1; [ $kern = duo ] && knob=QM_DUO_PARTS=-1
        for pass in sq tcc; do
          ctr="SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VMEM_RD SQ_INSTS_VALU SQ_INSTS_SALU"; [ $pass = tcc ] && ctr="TCC_REQ_sum TCC_HIT_sum TCC_MISS_sum"
          env ${lib:+QM_LIB_OVERRIDE=$lib} QM_SPLIT=1 $knob timeout -k 10 400 rocprofv3 --pmc $ctr --output-format csv -d "$OUT/pmc_${v}_${kern}_$pass" -o p -- python bench.py --gpus 1 --steps 1 --warmup 1 $QUIET > "$OUT/pmc_${v}_${kern}_$pass.log" 2>&1 || { tail -5 "$OUT/pmc_${v}_${kern}_$pass.log"; exit 1; }
        done
      done
    done ;;
  sum)  # the tables; of the profiler's output only this library's kernels' rows are kept
    python profiles/wave_runs/summarize.py "$OUT" --prune > "$OUT/summary.txt" 2>&1; cat "$OUT/summary.txt" ;;
  esac
done
