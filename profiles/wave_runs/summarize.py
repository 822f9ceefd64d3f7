#!/usr/bin/env python3
"""profiles/wave_runs/summarize.py OUT -- what run.sh left under OUT as text on stdout: the bench lines by variant, the per-kernel durations of
the two kernel traces, and per kernel and library the counters per dispatch and per pair with the slot fill
SQ_WAVE_CYCLES x 4 / SQ_BUSY_CYCLES / 256.  --prune: keep of the profiler's directories only the rows of this library's kernels
(OUT/raw/*.csv.gz) and drop the dumped arrays, so that OUT stays small."""
import collections
import csv
import glob
import gzip
import json
import os
import shutil
import statistics as st
import sys

OUT = sys.argv[1]
PRUNE = "--prune" in sys.argv[2:]
PAIRS = 1e7


def short(k):
    return k.split("(")[0].replace("void ", "").replace("qm::", "").split("<")[0]


def rows(pattern):
    """the rows of every csv under OUT that matches; after --prune: of the kept copy"""
    out = []
    for f in sorted(glob.glob(os.path.join(OUT, pattern), recursive=True)):
        with (gzip.open(f, "rt") if f.endswith(".gz") else open(f)) as h:
            out += list(csv.DictReader(h))
    return out


def keep(name, pattern):
    """the rows of this library's kernels of the csv files that match -> OUT/raw/name.csv.gz"""
    files = sorted(glob.glob(os.path.join(OUT, pattern), recursive=True))
    if not files:
        return
    os.makedirs(os.path.join(OUT, "raw"), exist_ok=True)
    with gzip.open(os.path.join(OUT, "raw", name + ".csv.gz"), "wt") as o:
        head = False
        for f in files:
            with open(f) as h:
                first = h.readline()
                if not head:
                    o.write(first)
                    head = True
                for line in h:
                    if "qm_" in line or "qm::" in line:
                        o.write(line)


def bench_tables():
    print("# bench.py lines by variant: M pairs/s (ms_per_step, map_kernel_ms), in the order they were measured")
    for f in sorted(glob.glob(os.path.join(OUT, "*.jsonl"))):
        v, ms, km = [], [], []
        for line in open(f):
            line = line.strip()
            if not line.startswith("{"):
                continue
            d = json.loads(line)
            v.append(d["value"]); ms.append(d["ms_per_step"]); km.append(d.get("config", {}).get("map_kernel_ms"))
        if not v:
            continue
        name = os.path.basename(f)[:-6]
        print("%-14s n %d  min %.1f  median %.1f  max %.1f  mean %.1f  spread %.1f M pairs/s;  ms_per_step median %.3f;  map_kernel_ms median %s"
              % (name, len(v), min(v), st.median(v), max(v), st.mean(v), max(v) - min(v), st.median(ms),
                 "%.3f" % st.median([k for k in km if k is not None]) if any(k is not None for k in km) else "-"))
        print("   " + "  ".join("%.1f (%.3f, %s)" % (a, b, c) for a, b, c in zip(v, ms, km)))


def trace_tables():
    for v in ("parent", "branch"):
        name = "trace_" + v
        r = rows("raw/%s.csv.gz" % name) or rows("%s/**/*kernel_trace.csv" % name)
        if not r:
            continue
        by = collections.defaultdict(list)
        for x in r:
            if "qm" in x["Kernel_Name"]:
                by[short(x["Kernel_Name"])].append((int(x["Start_Timestamp"]), int(x["End_Timestamp"])))
        print("# kernel trace, %s: python bench.py --gpus 1 --steps 10 --warmup 3 under rocprofv3 --kernel-trace --stats" % v)
        for k in sorted(by, key=lambda k: -sum(e - s for s, e in by[k])):
            d = [(e - s) / 1e6 for s, e in by[k]]
            print("   %-28s dispatches %4d  mean %8.3f ms  median %8.3f ms  total %9.3f ms" % (k, len(d), st.mean(d), st.median(d), sum(d)))
        duo, lean = sorted(by.get("qm_duo_kernel", [])), sorted(by.get("qm_lean_kernel", []))
        if duo and lean:
            # stage A of a step: the pair kernel's launch and the lean kernel's launch that overlaps it (the two parts in flight)
            spans = []
            for s, e in duo:
                over = [(ls, le) for ls, le in lean if ls < e and le > s]
                if over:
                    spans.append((max([e] + [le for ls, le in over]) - min([s] + [ls for ls, le in over])) / 1e6)
            if spans:
                print("   stage-A span (pair kernel with the lean launches that overlap it): n %d  mean %.3f ms  median %.3f ms" % (len(spans), st.mean(spans), st.median(spans)))


def pmc_tables():
    print("# counters per dispatch of each kernel alone over the 10 M pairs (QM_SPLIT=1; lean: QM_NO_DUO=1, pair: QM_DUO_PARTS=-1), per pair in brackets")
    for kern, kname in (("duo", "qm_duo_kernel"), ("lean", "qm_lean_kernel")):
        for v in ("parent", "branch"):
            tot, n = collections.Counter(), collections.Counter()
            for p in ("sq", "tcc"):
                name = "pmc_%s_%s_%s" % (v, kern, p)
                for x in rows("raw/%s.csv.gz" % name) or rows("%s/**/*counter_collection.csv" % name):
                    if short(x["Kernel_Name"]) == kname:
                        tot[x["Counter_Name"]] += float(x["Counter_Value"]); n[x["Counter_Name"]] += 1
            if not tot:
                continue
            per = {c: tot[c] / n[c] for c in tot}
            print("%s, %s (%d dispatches):" % (kname, v, max(n.values())))
            for c in sorted(per):
                print("   %-18s %16.0f  (%9.3f)" % (c, per[c], per[c] / PAIRS))
            if per.get("SQ_BUSY_CYCLES"):
                print("   slot fill SQ_WAVE_CYCLES x 4 / SQ_BUSY_CYCLES / 256 = %.4f" % (per["SQ_WAVE_CYCLES"] * 4 / per["SQ_BUSY_CYCLES"] / 256))


if PRUNE:
    for d in sorted(glob.glob(os.path.join(OUT, "trace_*")) + glob.glob(os.path.join(OUT, "pmc_*"))):
        if os.path.isdir(d):
            keep(os.path.basename(d), os.path.basename(d) + ("/**/*kernel_trace.csv" if "trace_" in d else "/**/*counter_collection.csv"))
            shutil.rmtree(d)
    for d in glob.glob(os.path.join(OUT, "dump_*")):
        if os.path.isdir(d):
            shutil.rmtree(d)
for part in (bench_tables, trace_tables, pmc_tables):
    try:
        part()
    except Exception as e:                                       # a table that cannot be made does not hide the others
        print("# %s: %s: %s" % (part.__name__, type(e).__name__, e))
