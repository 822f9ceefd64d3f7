"""Fold time of qm_eqc_add against the hits download it replaces, on the headline workload (bench.py config 2: dense index, 10 M pairs).

    python profiles/eq_classes/measure_fold.py [--root TREE] [--pairs N] [--runs 3] [--no-fold]

--root: the tree to import rapmap_amd / bench from (default: this one).  --no-fold: time qm_fetch_hits_pinned only -- what a tree without
the feature (the parent commit) can do.  The batch is mapped once, device-resident; then download and fold are timed in turn, --runs times
each: the download by the host clock around the synchronous call, the fold by HIP events on its stream (QM_EQC_STAT_LAST_FOLD_US: first launch to
last read-back, so its launches AND its read-backs) and by the host clock as well (*_host_ms).  The fold is timed three ways: into an empty table (every class is claimed and published), into a table that already holds
the batch's classes (the steady state of a run), and the latter without the per-wavefront aggregation (QM_EQC_NO_AGGREGATE=1).
One JSON line on stdout."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ap.add_argument("--pairs", type=int, default=10_000_000)
ap.add_argument("--genes", type=int, default=40000)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--no-fold", action="store_true")
ap.add_argument("--once", action="store_true", help="one steady-state fold and out (the run rocprofv3 --kernel-trace --stats wraps)")
a = ap.parse_args()
sys.path.insert(0, a.root)
sys.argv = sys.argv[:1]

import numpy as np          # noqa: E402
import torch                # noqa: E402
import bench                # noqa: E402
import rapmap_amd as ra     # noqa: E402

dev = torch.device("cuda:0")
idx = bench.build_or_reuse_index(a.genes, 42, 31, 0, 1, bench.default_cache())
qi = ra.QuasiIndex(idx)
mp = ra.QuasiMapper(qi, 0)
text, starts, lens = bench.load_text_to_gpu(qi, dev)
s1, s2, off = bench.make_reads_gpu(text, starts, lens, a.pairs, 43, dev)
torch.cuda.synchronize()
n = a.pairs
r = mp.map_device(n, s1.data_ptr(), off.data_ptr(), s2.data_ptr(), off.data_ptr(), 100, fetch=False)
nh = r.n_hits
L = ra.api.lib()
p_off = L.qm_pinned_alloc((n + 1) * 8); p_hits = L.qm_pinned_alloc(max(nh, 1) * 32)
assert p_off and p_hits


def fetch_ms():
    t = time.perf_counter()
    rc = L.qm_fetch_hits_pinned(mp._h, C.c_void_p(p_off), C.c_void_p(p_hits))
    assert rc == 0
    return (time.perf_counter() - t) * 1e3


def fold_ms(t):
    """(HIP events, host clock)"""
    t0 = time.perf_counter()
    t.add(mp)
    return t.stat(t.LAST_FOLD_US) / 1e3, (time.perf_counter() - t0) * 1e3


out = {"root": os.path.relpath(a.root), "pairs": n, "n_hits": nh, "download_bytes": 8 * (n + 1) + 32 * nh,
       # every 32-byte sector of the hit records is read whatever part of it is used: the records and offsets once at the rate an in-order sweep reaches
       "byte_floor_ms_at_6.0TBps": (8 * (n + 1) + 32 * nh) / 6.0e12 * 1e3, "map_kernel_ms": r.map_kernel_ms}
fetch_ms()                                                                # (first touch of the pinned pages)
if a.no_fold:
    out["fetch_hits_pinned_ms"] = [round(fetch_ms(), 3) for _ in range(a.runs)]
else:
    warm = ra.EqClasses(mp, expected=1 << 20); warm.add(mp)                # scratch buffers sized, classes in place
    if a.once:
        fold_ms(warm)
        print(json.dumps({"once": True, "n_classes": warm.n_classes})); sys.exit(0)
    os.environ["QM_EQC_NO_AGGREGATE"] = "1"
    plain = ra.EqClasses(mp, expected=1 << 20); plain.add(mp)
    del os.environ["QM_EQC_NO_AGGREGATE"]
    f, cold, steady, noagg = [], [], [], []
    for _ in range(a.runs):
        f.append(fetch_ms())
        warm.clear(); cold.append(fold_ms(warm))
        steady.append(fold_ms(warm))
        noagg.append(fold_ms(plain))
    out.update(fetch_hits_pinned_ms=[round(x, 3) for x in f], fold_empty_table_ms=[round(x[0], 3) for x in cold],
               fold_steady_ms=[round(x[0], 3) for x in steady], fold_steady_no_aggregate_ms=[round(x[0], 3) for x in noagg],
               fold_empty_table_host_ms=[round(x[1], 3) for x in cold], fold_steady_host_ms=[round(x[1], 3) for x in steady],
               n_classes=warm.n_classes, n_tids=int(warm.fetch()[0][-1]), total=warm.total,
               rounds_last_table=warm.stat(warm.ROUNDS), growths=warm.stat(warm.GROWTHS), long_units=warm.stat(warm.LONG_UNITS),
               collision_probes=warm.stat(warm.COLLISION_PROBES))
    ho = np.ctypeslib.as_array(C.cast(p_off, C.POINTER(C.c_int64)), shape=(n + 1,))
    assert warm.total == 2 * int(np.count_nonzero(np.diff(ho))), "the table does not hold the batch twice"
print(json.dumps(out))
