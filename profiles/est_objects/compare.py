"""profiles/est_objects/compare.py -- the alternated runs of parent and branch side by side: per figure the parent's spread (min .. max over
all its runs' values) and the branch's median, and whether the median lies within the spread.
  python profiles/est_objects/compare.py profiles/est_objects/results > profiles/est_objects/results/side_by_side.txt
Reads {bench,fld,lib,fold}_{parent,branch}.jsonl: the last lines of bench.py, profiles/fld/measure_fld.py, profiles/lib/measure_lib.py and
profiles/eq_classes/measure_fold.py, one line per run, in the order they ran."""
import json
import statistics
import sys

FIGURES = {"bench": [("value",), ("ms_per_step",)],
           "fld": [("fold_ms", "default"), ("fold_ms", "256"), ("fold_ms", "1024"), ("fold_ms", "4096")],
           "lib": [("lib_add_ms", "IU"), ("lib_add_ms", "A"), ("eqc_add_lib_wall_ms", "IU"), ("eqc_add_lib_wall_ms", "ISF"), ("eqc_add_lib_sweep_ms", "IU"),
                   ("eqc_add_lib_sweep_ms", "ISF"), ("eqc_add_wall_ms",)],
           "fold": [("fold_empty_table_ms",), ("fold_steady_ms",), ("fold_steady_host_ms",)]}


def values(path, key):
    out = []
    for line in open(path):
        d = json.loads(line)
        for k in key:
            d = d[k]
        out += d if isinstance(d, list) else [d]
    return out


def main(root):
    print("%-34s %-22s %-10s %s" % ("figure", "parent min .. max", "branch med", "within"))
    for what, keys in FIGURES.items():
        for key in keys:
            p = values("%s/%s_parent.jsonl" % (root, what), key); b = values("%s/%s_branch.jsonl" % (root, what), key)
            med = statistics.median(b)
            print("%-34s %-22s %-10.4g %s   (parent median %.4g, %d / %d values)" % (what + " " + ".".join(key), "%.4g .. %.4g" % (min(p), max(p)), med,
                                                                                  "yes" if min(p) <= med <= max(p) else "NO", statistics.median(p), len(p), len(b)))


if __name__ == "__main__":
    main(sys.argv[1])
