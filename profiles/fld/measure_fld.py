"""Fold time of qm_fld_add on the headline workload (bench.py config 2: dense index, 10 M pairs), beside its byte floor and beside the
steady fold of qm_eqc_add over the same batch in the same process.

    python profiles/fld/measure_fld.py [--pairs N] [--runs 3] [--caps 0,256,1024,4096]

The batch is mapped once, device-resident.  Per cap on the number of workgroups (0: the default grid) one warm-up fold, then --runs
folds timed by HIP events on the fold's stream (QM_FLD_STAT_LAST_FOLD_US: the kernel alone).  The byte floor: all offsets once and one
whole 32-byte sector per single-hit unit, at 6.0 TB/s.  Every histogram is held against the first one: the grid must not matter.
One JSON line on stdout."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=10_000_000)
ap.add_argument("--genes", type=int, default=40000)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--caps", default="0,256,1024,4096")
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
out = {"pairs": n, "n_hits": r.n_hits, "map_kernel_ms": r.map_kernel_ms, "fold_ms": {}}
first = None
for cap in (int(x) for x in a.caps.split(",")):
    f = ra.FragLenDist(mp, max_blocks=cap)
    f.add(mp)                                                            # warm-up
    ms = []
    for _ in range(a.runs):
        f.add(mp); ms.append(round(f.stat()["last_fold_us"] / 1e3, 3))
    st = f.stat(); c = f.counts()
    assert st["units"] == (a.runs + 1) * n and sum(st[k] for k in ra.FLD_STATS[1:]) == st["units"]
    if first is None:
        first = c
        single = (st["units"] - st["unmapped"] - st["multi"]) // (a.runs + 1)
        out.update(stats_per_fold={k: st[k] // (a.runs + 1) for k in ra.FLD_STATS}, mean_frag_len=f.mean(), single_hit_units=single,
                   byte_floor_ms_at_6_0TBps=round((8 * (n + 1) + 32 * single) / 6.0e12 * 1e3, 4))
    assert np.array_equal(c, first), "the histogram depends on the grid"
    out["fold_ms"]["default" if cap == 0 else str(cap)] = ms
    f.close()
t = ra.EqClasses(mp, expected=1 << 20); t.add(mp)                        # classes in place: the steady state of a run
eq = []
for _ in range(a.runs):
    t.add(mp); eq.append(round(t.stat(t.LAST_FOLD_US) / 1e3, 3))
out["eqc_steady_fold_ms"] = eq
print(json.dumps(out))
