"""Sweep time of qm_lib_add and fold time of qm_eqc_add_lib on the headline workload (bench.py config 2: dense index, 10 M pairs), beside
the plain fold of qm_eqc_add over the same batch in the same process, and beside the byte floor.

    python profiles/lib/measure_lib.py [--pairs N] [--runs 3]

The batch is mapped once, device-resident.  After one warm-up of each, --runs turns, alternating in one process: (a) qm_lib_add under
IU and under the all-codes mask (QM_LIB_STAT_LAST_SWEEP_US: first launch to last, by HIP events on the context's stream), (b)
qm_eqc_add_lib under IU and under ISF and qm_eqc_add, each into a table of its own that holds its classes (wall time around the call,
the stream idle before and after; QM_EQC_STAT_LAST_FOLD_US for the fold inside it).  (c) The byte floor of the sweep: all offsets once
and one whole 32-byte sector per hit, at 6.0 TB/s.  The tallies of every turn are held against the first one's: the order of the
wavefronts must not matter.  One JSON line on stdout."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=10_000_000)
ap.add_argument("--genes", type=int, default=40000)
ap.add_argument("--runs", type=int, default=3)
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
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
out = {"pairs": n, "n_hits": r.n_hits, "map_kernel_ms": r.map_kernel_ms,
       "byte_floor_ms_at_6_0TBps": round((8 * (n + 1) + 32 * r.n_hits) / 6.0e12 * 1e3, 4)}

sweeps = {t: ra.LibFormat(mp, t) for t in ("IU", "A")}
folds = {t: (ra.LibFormat(mp, t), ra.EqClasses(mp, expected=1 << 20)) for t in ("IU", "ISF")}
plain = ra.EqClasses(mp, expected=1 << 20)
for L in sweeps.values():
    L.add(mp)                                                            # warm-up
for L, t in folds.values():
    t.add(mp, lib=L)                                                     # warm-up: the classes are in place
plain.add(mp)
first = {k: L.counts() for k, L in sweeps.items()}
first.update({"fold " + k: L.counts() for k, (L, t) in folds.items()})
res = {"lib_add_ms": {k: [] for k in sweeps}, "eqc_add_lib_wall_ms": {k: [] for k in folds}, "eqc_add_lib_sweep_ms": {k: [] for k in folds},
       "eqc_add_lib_fold_ms": {k: [] for k in folds}, "eqc_add_wall_ms": [], "eqc_add_fold_ms": []}


def wall(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); return round((time.perf_counter() - t0) * 1e3, 3)


for i in range(a.runs):
    for k, L in sweeps.items():
        L.add(mp); res["lib_add_ms"][k].append(round(L.stat()["last_sweep_us"] / 1e3, 3))
        assert np.array_equal(L.counts(), first[k] * np.uint64(i + 2)), "the tallies depend on the order of the wavefronts"
    for k, (L, t) in folds.items():
        res["eqc_add_lib_wall_ms"][k].append(wall(lambda: t.add(mp, lib=L)))
        res["eqc_add_lib_sweep_ms"][k].append(round(L.stat()["last_sweep_us"] / 1e3, 3)); res["eqc_add_lib_fold_ms"][k].append(round(t.stat(t.LAST_FOLD_US) / 1e3, 3))
        assert np.array_equal(L.counts(), first["fold " + k] * np.uint64(i + 2))
    res["eqc_add_wall_ms"].append(wall(lambda: plain.add(mp))); res["eqc_add_fold_ms"].append(round(plain.stat(plain.LAST_FOLD_US) / 1e3, 3))
out.update(res)
out["tally_per_sweep_IU"] = ra.lib_format_counts(first["IU"], "IU")
out["classes"] = {"plain": plain.n_classes, **{k: t.n_classes for k, (L, t) in folds.items()}}
out["lib_add_over_floor"] = {k: round(min(v) / out["byte_floor_ms_at_6_0TBps"], 2) for k, v in res["lib_add_ms"].items()}
print(json.dumps(out))
