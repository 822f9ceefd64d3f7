"""Bootstrap replicates on the headline workload (bench.py config 2: dense index, one mapped batch of 10 M pairs; the table that
profiles/quant/measure_quant.py builds).

    python profiles/boot/measure_boot.py [--pairs N] [--iters 1000] [--runs 3] [--reps 1,16,64,128] [--conv 100] [--what abc]

  (a) resample: time per replicate (N draws each) by HIP events on the stream (QM_BOOT_STAT_LAST_RESAMPLE_US), 16 replicates, with and
      without the per-wavefront aggregation (QM_BOOT_AGGREGATE read at create), three turns each; counts held equal between the two;
  (b) time per iteration per replicate for --reps replicates at rel_tol = 0 (no read-back inside the run), --iters iterations, --runs
      turns; beside it Quant's own time per iteration in the same process, and the byte floor of one iteration per replicate worked out
      as DESIGN.md section 4.10 does: index entries read once PER TILE of 16 replicates (4 bytes each, both sides), counts read, w, r
      and alpha read and written once per replicate, at 6.0 TB/s;
  (c) convergence at the defaults: --conv replicates end to end (resample + run + fetch, host clock) against --conv successive Quant
      runs from the uniform start on the same graph (a Quant holds the original counts: its run is what one replicate costs alone).
One JSON line on stdout."""
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
ap.add_argument("--reps", default="1,16,64,128")
ap.add_argument("--conv", type=int, default=100)
ap.add_argument("--what", default="abc")
a = ap.parse_args()
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
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
r = mp.map_device(a.pairs, s1.data_ptr(), off.data_ptr(), s2.data_ptr(), off.data_ptr(), 100, fetch=False)
table = ra.EqClasses(mp, expected=1 << 20)
table.add(mp)
del s1, s2, off
nt = qi.n_txps
eff = np.asarray(qi.txp_lens, dtype=np.float64)
q = ra.Quant(table, nt, eff)
st = q.stat()
E, nc = st["entries"], st["classes"]
out = {"pairs": a.pairs, "n_txps": nt, "quant_stat": st, "total": table.total}


def flush():
    print(json.dumps(out), flush=True)


if "a" in a.what:                                                         # (a)
    res = {}
    counts = {}
    for flag in ("0", "1"):
        os.environ["QM_BOOT_AGGREGATE"] = flag
        b = ra.Bootstrap(q, 16)
        del os.environ["QM_BOOT_AGGREGATE"]
        b.resample(seed=1)                                                # (warm-up: code objects loaded)
        us = []
        for turn in range(a.runs):
            b.resample(seed=1, first_rep=16 * turn)
            us.append(b.stat()["last_resample_us"] / 16)
        counts[flag] = b.counts(5)
        res["aggregate_" + flag + "_us_per_replicate"] = [round(x, 1) for x in us]
        out["boot_stat"] = b.stat()
        b.close()
    assert np.array_equal(counts["0"], counts["1"]) and int(counts["0"].sum()) == table.total
    res["draws_per_replicate"] = int(table.total)
    out["a_resample"] = res
    flush()

if "b" in a.what:                                                         # (b)
    q.run(max_iter=20, rel_tol=0.0)
    per = []
    for _ in range(a.runs):
        q.set_start(None)
        it, _ = q.run(max_iter=a.iters, rel_tol=0.0)
        per.append(q.stat()["last_run_us"] / a.iters)
    out["b_iterations"] = a.iters
    out["b_quant_us_per_iteration"] = [round(x, 3) for x in per]
    qb = 4 * E + 4 * E + 2 * 8 * (nt + nc + nt)
    out["b_quant_byte_floor_us_at_6.0TBps"] = round(qb / 6.0e12 * 1e6, 3)
    rows = {}
    for n in [int(x) for x in a.reps.split(",")]:
        b = ra.Bootstrap(q, n)
        tiles = (n + 15) // 16
        b.resample(seed=2)
        b.run(max_iter=20, rel_tol=0.0)
        us = []
        for _ in range(a.runs):
            b.resample(seed=2)
            it, _ = b.run(max_iter=a.iters, rel_tol=0.0)
            assert it.tolist() == [a.iters] * n
            us.append(b.stat()["last_run_us"] / a.iters)
        # per iteration: the index arrays once per tile; per replicate cnt (8) read, single (8) read, w read + written (class side reads it
        # through the gather, the transcript side reads and writes its own), r written + gathered, alpha written
        bytes_it = tiles * (4 * E + 4 * E) + n * (8 * nc + 8 * nt + 2 * 8 * (nt + nc) + 8 * nt)
        rows[str(n)] = {"us_per_iteration": [round(x, 3) for x in us], "us_per_iteration_per_replicate": [round(x / n, 3) for x in us],
                        "byte_floor_us_per_replicate_at_6.0TBps": round(bytes_it / n / 6.0e12 * 1e6, 3), "launches": b.stat()["launches"]}
        b.close()
    out["b_boot"] = rows
    flush()

if "c" in a.what:                                                         # (c)
    n = a.conv
    t0 = time.perf_counter()
    its, us = [], 0
    for first in range(0, n, 64):
        b = ra.Bootstrap(q, min(64, n - first))
        b.resample(seed=3, first_rep=first)
        it, rel = b.run()
        al = b.fetch()
        s = b.stat(); us += s["last_resample_us"] + s["last_run_us"]
        its += it.tolist()
        b.close()
    boot_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    qits = []
    for _ in range(n):
        q.set_start(None)
        it, rel = q.run()
        q.fetch()
        qits.append(it)
    quant_ms = (time.perf_counter() - t0) * 1e3
    out["c_convergence"] = {"replicates": n, "boot_ms_host_clock": round(boot_ms, 1), "boot_ms_hip_events": round(us / 1e3, 1),
                            "boot_iterations_min_median_max": [int(min(its)), int(np.median(its)), int(max(its))],
                            "successive_quant_ms_host_clock": round(quant_ms, 1), "quant_iterations": int(qits[0]),
                            "note": "the Quant runs hold the ORIGINAL counts (no resample): what one replicate costs alone, without the draws"}
    flush()
q.close()
