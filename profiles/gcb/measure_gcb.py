"""The GC bias kernels on the headline workload (bench.py config 2: dense index, 10 M pairs): (a) the observed sweep beside qm_fld_add in
the same process and beside its byte floor, (b) qm_gcb_expect with that run's fragment-length histogram -- time, windows evaluated,
the issue floor that follows from the vector instructions per step, and the numpy restatement's time on a sample of transcripts --,
(c) the build of the rank structure.

    python profiles/gcb/measure_gcb.py [--pairs N] [--runs 3] [--sample 300]

The batch is mapped once, device-resident.  One warm-up, then --runs turns timed by HIP events on the kernel's stream
(QM_GCB_STAT_LAST_FOLD_US / LAST_EXPECT_US / RANK_BUILD_US).  Every turn's counts are held against the first turn's.  One JSON line."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=10_000_000)
ap.add_argument("--genes", type=int, default=40000)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--sample", type=int, default=300)
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
n = a.pairs
r = mp.map_device(n, s1.data_ptr(), off.data_ptr(), s2.data_ptr(), off.data_ptr(), 100, fetch=False)
out = {"pairs": n, "n_hits": r.n_hits, "text_len": int(text.numel()), "n_txps": qi.n_txps}

g = ra.GCBias(mp)
out["rank_build_ms"] = g.stat()["rank_build_us"] / 1e3                   # (c): this object built the replica's structure
f = ra.FragLenDist(mp)
g.add(mp); f.add(mp)                                                     # warm-up
first = g.counts()
sweep, fold = [], []
for _ in range(a.runs):                                                  # (a): in turn, in one process
    g.add(mp); sweep.append(round(g.stat()["last_fold_us"] / 1e3, 3))
    f.add(mp); fold.append(round(f.stat()["last_fold_us"] / 1e3, 3))
st = g.stat()
assert np.array_equal(g.counts(), first * np.uint64(a.runs + 1)), "the observed counts differ from turn to turn"
per = {k: st[k] // (a.runs + 1) for k in ra.GCB_STATS}
single = per["units"] - per["unmapped"] - per["multi"]
# the byte floor: all offsets once, one 32-byte sector per single-hit unit, and per used or overhanging unit txpOff and txpLen (a
# sector each: gathers) and, for a used one, two mask words and two rank words (four sectors)
floor = (8 * (n + 1) + 32 * single + 64 * (per["used"] + per["overhang"]) + 128 * per["used"]) / 6.0e12 * 1e3
out.update(obs_sweep_ms=sweep, fld_fold_ms=fold, stats_per_sweep=per, obs=[int(x) for x in first], sweep_byte_floor_ms_at_6_0TBps=round(floor, 4))

fc = f.counts() // np.uint64(a.runs + 1)                                 # (b): that run's fragment lengths
T = qi.n_txps
H0 = g.expect(fc, T)                                                     # warm-up (builds the tile table)
ex = []
for _ in range(a.runs):
    H = g.expect(fc, T); ex.append(round(g.stat()["last_expect_us"] / 1e3, 3))
    assert H.tobytes() == H0.tobytes(), "the expected matrix differs from turn to turn"
L = np.asarray(qi.txp_lens, dtype=np.int64)
ls = np.flatnonzero(fc)
windows = int(sum(int(np.maximum(L - l + 1, 0).sum()) for l in ls))
out.update(expect_ms=ex, lengths_with_counts=int(ls.size), windows=windows,
           # 5 vector instructions per counted step and 10 per turn of the fold (results/expect_inner_loop.s), a wavefront step
           # covers 64 windows; 256 CUs x 4 SIMDs at 2.4 GHz, a 64-lane vector instruction occupying its 16-lane SIMD for four cycles
           issue_floor_ms_by_fold_turns={str(k): round(windows / 64 * (5 + 10 * k) * 4 / (256 * 4 * 2.4e9) * 1e3, 3) for k in (1, 2, 3)})
import gcb_cases as gcc     # noqa: E402
txt, offs = qi.arrays()
pick = np.linspace(0, T - 1, min(a.sample, T)).astype(np.int64)
w = {"text": txt, "off": offs[pick], "lens": L[pick]}
t0 = time.time()
Hs = gcc.expect(w, fc)
dt = time.time() - t0
assert np.array_equal(Hs, H0[pick]), "the device's rows differ from the restatement's"
gcc.assert_identity({"lens": L}, fc, H0, "config 2")
out.update(restatement_sample_txps=int(pick.size), restatement_sample_s=round(dt, 3),
           restatement_all_s_extrapolated=round(dt * float(L.sum()) / float(L[pick].sum()), 1))
print(json.dumps(out))
