"""profiles/est_objects/compare.py -- the alternated runs of parent and branch side by side: per figure the parent's spread (min .. max over
all its runs' values) and the branch's median, and whether the median is no worse than the spread: a time at or below the parent's maximum,
a rate (bench value) at or above its minimum.
  python profiles/est_objects/compare.py profiles/est_objects/results > profiles/est_objects/results/side_by_side.txt
Reads {bench,fld,lib,fold,gcb}_{parent,branch}.jsonl: the last lines of bench.py, profiles/fld/measure_fld.py, profiles/lib/measure_lib.py,
profiles/eq_classes/measure_fold.py and profiles/gcb/measure_gcb.py, one line per run, in the order they ran; a kind without files is left out."""
import json
import os
import statistics
import sys

FIGURES = {"bench": [("value",), ("ms_per_step",)],
           "fld": [("fold_ms", "default"), ("fold_ms", "256"), ("fold_ms", "1024"), ("fold_ms", "4096")],
           "lib": [("lib_add_ms", "IU"), ("lib_add_ms", "A"), ("eqc_add_lib_wall_ms", "IU"), ("eqc_add_lib_wall_ms", "ISF"), ("eqc_add_lib_sweep_ms", "IU"),
                   ("eqc_add_lib_sweep_ms", "ISF"), ("eqc_add_wall_ms",)],
           "fold": [("fold_empty_table_ms",), ("fold_steady_ms",), ("fold_steady_host_ms",)],
           "gcb": [("obs_sweep_ms",), ("expect_ms",), ("rank_build_ms",)]}
HIGHER_IS_BETTER = {("bench", ("value",))}


def values(path, key):
    out = []
    for line in open(path):
        d = json.loads(line)
        for k in key:
            d = d[k]
        out += d if isinstance(d, list) else [d]
    return out


def main(root):
    print("%-34s %-22s %-10s %s" % ("figure", "parent min .. max", "branch med", "no worse"))
    for what, keys in FIGURES.items():
        if not os.path.exists("%s/%s_parent.jsonl" % (root, what)):
            continue
        for key in keys:
            p = values("%s/%s_parent.jsonl" % (root, what), key); b = values("%s/%s_branch.jsonl" % (root, what), key)
            med = statistics.median(b)
            print("%-34s %-22s %-10.4g %s   (parent median %.4g, %d / %d values)" % (what + " " + ".".join(key), "%.4g .. %.4g" % (min(p), max(p)), med,
                                                                                  "yes" if (med >= min(p) if (what, key) in HIGHER_IS_BETTER else med <= max(p)) else "NO", statistics.median(p), len(p), len(b)))


if __name__ == "__main__":
    main(sys.argv[1])
