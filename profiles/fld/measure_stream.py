"""FASTQ -> classes through the stream without hits (QM_STREAM_EQ_CLASSES | QM_STREAM_NO_HITS), with and without QM_STREAM_FLD.

    python profiles/fld/measure_stream.py [--fld] --fq1 F1 --fq2 F2

The files are the ones profiles/eq_classes/measure_stream.py --write makes.  open_to_last_result_s: from before the stream is opened
until the class table (and, with --fld, the histogram) is in host memory.  One JSON line."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--fld", action="store_true")
ap.add_argument("--fq1", required=True); ap.add_argument("--fq2", required=True)
ap.add_argument("--genes", type=int, default=40000)
ap.add_argument("--threads", type=int, default=16)
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.argv = sys.argv[:1]

import bench                # noqa: E402
import rapmap_amd as ra     # noqa: E402

idx = bench.build_or_reuse_index(a.genes, 42, 31, 0, 1, bench.default_cache())
qi = ra.QuasiIndex(idx)
ra.reserve_stream_memory(1280 << 20)
keep = ra.QuasiMapper(qi, 0)                                               # the replica stays; the stream's contexts share it
t0 = time.perf_counter()
st = ra.MappedStream(qi, a.fq1, a.fq2, batch_units=1 << 18, threads=a.threads, names=False, eq_classes=True, hits=False, frag_len_dist=a.fld)
units = hits = 0
for b in st:
    units += b.n; hits += b.n_hits
o, t, c = st.eq_classes()
out = {"fld": a.fld, "pairs": units, "n_hits": hits, "n_classes": len(c), "total": int(c.sum())}
if a.fld:
    counts, stats = st.frag_len_dist()
    out.update(fld_stats=stats, mean_frag_len=ra.frag_len_mean(counts))
out["open_to_last_result_s"] = round(time.perf_counter() - t0, 4)
ss = st.stats()
out.update(fold_s=round(ss["fold_s"], 4), fld_fold_s=round(ss["fld_fold_s"], 4))
st.close()
print(json.dumps(out))
