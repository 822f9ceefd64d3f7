"""profiles/estim_driver/compare.py -- parent and branch side by side from the lines that measure_fold.py, measure_quant.py and
measure_boot.py wrote, one line per process and tree (DIR/{fold,quant,boot}_{parent,branch}.jsonl).  Per figure: every process's
median of its own turns, the parent's spread over its processes, the branch's median over its processes, and whether that median
lies within the parent's spread.
  python profiles/estim_driver/compare.py DIR"""
import json
import os
import statistics as st
import sys

D = sys.argv[1]


def lines(name):
    p = os.path.join(D, name)
    return [json.loads(x) for x in open(p)] if os.path.exists(p) else []


FIGURES = (
    ("fold", "fold into a table that holds the classes, ms per batch", lambda d: d["fold_steady_ms"]),
    ("fold", "fold into an empty table, ms per batch", lambda d: d["fold_empty_table_ms"]),
    ("quant", "quant build, us (the first create of a process left out)", lambda d: [1e3 * x for x in d["a_build_ms_hip_events"][1:]]),
    ("quant", "quant, us per iteration", lambda d: d["b_us_per_iteration_hip_events"]),
    ("boot", "boot resample, us per replicate (aggregate 0)", lambda d: d["a_resample"]["aggregate_0_us_per_replicate"]),
    ("boot", "boot resample, us per replicate (aggregate 1)", lambda d: d["a_resample"]["aggregate_1_us_per_replicate"]),
) + tuple(("boot", "boot, us per iteration per replicate, %s replicates" % n, (lambda n: lambda d: d["b_boot"][n]["us_per_iteration_per_replicate"])(n)) for n in ("1", "16", "64", "128"))

for which, what, get in FIGURES:
    par = [st.median(get(d)) for d in lines(which + "_parent.jsonl")]
    br = [st.median(get(d)) for d in lines(which + "_branch.jsonl")]
    if not par or not br:
        continue
    m = st.median(br)
    print("%-62s parent %s (spread %.4g .. %.4g)  branch %s (median %.4g)  %s" % (
        what, " / ".join("%.4g" % x for x in par), min(par), max(par), " / ".join("%.4g" % x for x in br), m,
        "within" if min(par) <= m <= max(par) else "below" if m < min(par) else "ABOVE by %.2f %%" % (100 * (m / max(par) - 1))))
for tree in ("parent", "branch"):
    for d in lines("bench_%s.jsonl" % tree):
        print("bench.py --gpus 1 --steps 8 --warmup 2, %s: %s" % (tree, json.dumps({k: d[k] for k in d if k in ("value", "unit", "metric", "ms_per_step", "pairs_per_s", "mpairs_per_s")} or d)[:300]))
