"""The EM over the equivalence-class table on the headline workload (bench.py config 2: dense index, one mapped batch of 10 M pairs).

    python profiles/quant/measure_quant.py [--pairs N] [--iters 1000] [--runs 3]

The batch is mapped once, device-resident, and folded into a table where it lies; then
  (a) the structure build of a quant object (QM_QUANT_STAT_BUILD_US: HIP events on its stream around mark .. queues, read-backs included),
      and the host clock around the whole create;
  (b) --iters iterations at rel_tol = 0 (no read-back inside the run), --runs turns from the uniform start, by HIP events on the
      object's stream (QM_QUANT_STAT_LAST_RUN_US) -> time per iteration; beside it the byte floor of one iteration -- label entries and
      transposed entries (4 bytes each) read once, w, r and alpha (8 bytes each) read and written once, at the 6.0 TB/s an in-order
      sweep reaches -- and the numpy restatement's time per iteration on this host (tests/quant_cases.py);
  (c) a run at the defaults (max_iter 10000, check_every 10, rel_tol 1e-2, min_alpha 1e-8): iterations, HIP-event time, host clock.
Five iterations are also held against the restatement (quant_cases.assert_close).  One JSON line on stdout."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=10_000_000)
ap.add_argument("--genes", type=int, default=40000)
ap.add_argument("--iters", type=int, default=1000)
ap.add_argument("--runs", type=int, default=3)
a = ap.parse_args()
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.argv = sys.argv[:1]

import numpy as np          # noqa: E402
import torch                # noqa: E402
import bench                # noqa: E402
import rapmap_amd as ra     # noqa: E402
import quant_cases as qc    # noqa: E402

dev = torch.device("cuda:0")
idx = bench.build_or_reuse_index(a.genes, 42, 31, 0, 1, bench.default_cache())
qi = ra.QuasiIndex(idx)
mp = ra.QuasiMapper(qi, 0)
text, starts, lens = bench.load_text_to_gpu(qi, dev)
s1, s2, off = bench.make_reads_gpu(text, starts, lens, a.pairs, 43, dev)
torch.cuda.synchronize()
r = mp.map_device(a.pairs, s1.data_ptr(), off.data_ptr(), s2.data_ptr(), off.data_ptr(), 100, fetch=False)
table = ra.EqClasses(mp, expected=1 << 20)
table.add(mp)
nt = qi.n_txps
eff = np.asarray(qi.txp_lens, dtype=np.float64)

build_us, create_ms = [], []
q = None
for _ in range(a.runs):                                                   # (a)
    if q is not None:
        q.close()
    t0 = time.perf_counter()
    q = ra.Quant(table, nt, eff)
    create_ms.append((time.perf_counter() - t0) * 1e3)
    build_us.append(q.stat()["build_us"])
st = q.stat()
E, nc = st["entries"], st["classes"]
floor_bytes = 4 * E + 4 * E + 2 * 8 * (nt + nc + nt)
out = {"pairs": a.pairs, "n_hits": r.n_hits, "n_txps": nt, "stat": st, "total": table.total,
       "a_build_ms_hip_events": [round(x / 1e3, 3) for x in build_us], "a_create_ms_host_clock": [round(x, 3) for x in create_ms],
       "b_bytes_per_iteration": floor_bytes, "b_byte_floor_us_at_6.0TBps": round(floor_bytes / 6.0e12 * 1e6, 3)}

q.run(max_iter=20, rel_tol=0.0)                                           # (warm-up: code objects loaded, clocks up)
per_iter = []
for _ in range(a.runs):                                                   # (b)
    q.set_start(None)
    it, _ = q.run(max_iter=a.iters, rel_tol=0.0)
    assert it == a.iters
    per_iter.append(q.stat()["last_run_us"] / a.iters)
out["b_iterations"] = a.iters
out["b_us_per_iteration_hip_events"] = [round(x, 3) for x in per_iter]

g = qc.Graph(*table.fetch(), nt)
a0 = g.uniform_start()
qc.step(g, eff, a0)
t0 = time.perf_counter()
ref = qc.iterate(g, eff, a0, 5)
out["b_numpy_restatement_ms_per_iteration"] = round((time.perf_counter() - t0) * 1e3 / 5, 3)
q.set_start(None); q.run(max_iter=5, rel_tol=0.0)
qc.assert_close(q.fetch(), ref, "config 2, 5 iterations")

conv = []
for _ in range(a.runs):                                                   # (c)
    q.set_start(None)
    t0 = time.perf_counter()
    it, rel = q.run()
    conv.append({"iterations": it, "last_rel_change": rel, "ms_hip_events": round(q.stat()["last_run_us"] / 1e3, 3),
                 "ms_host_clock": round((time.perf_counter() - t0) * 1e3, 3)})
out["c_defaults"] = conv
alpha = q.fetch()
out["c_sum_alpha_over_total_minus_1"] = float(alpha.sum()) / table.total - 1.0
print(json.dumps(out))
