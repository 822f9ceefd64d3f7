"""The variational Bayes EM beside the EM on the headline workload (bench.py config 2: dense index, one mapped batch of 10 M pairs).

    python profiles/vb/measure_vb.py [--pairs N] [--iters 1000] [--runs 3]

The batch is mapped once, device-resident, and folded into a table where it lies; one quant object serves both methods (set_method
between the turns), effective length = length, the default prior (1e-2 per nucleotide).
  (a) --iters iterations at rel_tol = 0 (no read-back inside the run), --runs turns per method in alternation from the uniform start,
      by HIP events on the object's stream (QM_QUANT_STAT_LAST_RUN_US) -> time per iteration, their ratio, and the byte floor of one
      iteration as profiles/quant/measure_quant.py counts it (the variational step reads the prior as well: 8 bytes per transcript);
  (b) a run at the defaults (max_iter 10000, check_every 10, rel_tol 1e-2, min_alpha 1e-8) per method: iterations, HIP-event time,
      and the transcripts that end above min_alpha.
Five variational iterations are also held against the restatement (vb_cases.assert_close).  One JSON line on stdout."""
import argparse
import json
import os
import sys

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
import vb_cases as vc       # noqa: E402

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
q = ra.Quant(table, nt, eff)
st = q.stat()
E, nc = st["entries"], st["classes"]
floor_em = 4 * E + 4 * E + 2 * 8 * (nt + nc + nt)
floor_vb = floor_em + 8 * nt
METHODS = (("em", {}), ("vbem", {"prior": 1e-2, "per_transcript": False}))
out = {"pairs": a.pairs, "n_hits": r.n_hits, "n_txps": nt, "stat": st, "total": table.total, "a_iterations": a.iters,
       "a_byte_floor_us_at_6.0TBps": {"em": round(floor_em / 6.0e12 * 1e6, 3), "vbem": round(floor_vb / 6.0e12 * 1e6, 3)}}

for m, kw in METHODS:                                                     # (warm-up: code objects loaded, clocks up)
    q.set_method(m, **kw); q.run(max_iter=20, rel_tol=0.0)
per_iter = {"em": [], "vbem": []}
for _ in range(a.runs):                                                   # (a)
    for m, kw in METHODS:
        q.set_method(m, **kw); q.set_start(None)
        it, _ = q.run(max_iter=a.iters, rel_tol=0.0)
        assert it == a.iters
        per_iter[m].append(q.stat()["last_run_us"] / a.iters)
out["a_us_per_iteration_hip_events"] = {m: [round(x, 3) for x in v] for m, v in per_iter.items()}
out["a_ratio_vbem_over_em_of_medians"] = round(float(np.median(per_iter["vbem"]) / np.median(per_iter["em"])), 4)

g = qc.Graph(*table.fetch(), nt)
prior = vc.prior_of(1e-2, False, eff, nt)
q.set_method("vbem", prior=prior); q.set_start(None); q.run(max_iter=5, rel_tol=0.0)
vc.assert_close(q.fetch(), vc.iterate(g, eff, prior, g.uniform_start(), 5), "config 2, 5 variational iterations")

conv = {"em": [], "vbem": []}
for _ in range(a.runs):                                                   # (b)
    for m, kw in METHODS:
        q.set_method(m, **kw); q.set_start(None)
        it, rel = q.run()
        alpha = q.fetch()
        conv[m].append({"iterations": it, "last_rel_change": rel, "ms_hip_events": round(q.stat()["last_run_us"] / 1e3, 3),
                        "above_min_alpha": int((alpha > ra.Quant.DEFAULTS["min_alpha"]).sum()), "present": st["present"],
                        "sum_alpha_over_total_minus_1": float(alpha.sum()) / table.total - 1.0})
out["b_defaults"] = conv
print(json.dumps(out))
