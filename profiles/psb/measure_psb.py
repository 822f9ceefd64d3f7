"""The positional bias kernels on the headline workload (bench.py config 2: dense index, 10 M pairs): (a) the observed sweep beside
qm_fld_add, qm_gcb_add and qm_sqb_add on the same batch, in turn, and beside its byte floor; (b) qm_psb_expect with that run's
fragment-length histogram and weights from a flat first estimate, the two-end identity checked on the full index; (c) qm_psb_eff_lens
and qm_sqb_eff_lens on the same histogram, in turn, each with its own model's ratios, and equality of the positional one with the numpy
restatement on a sample of transcripts.

    python profiles/psb/measure_psb.py [--pairs N] [--runs 3] [--sample 300]

The batch is mapped once, device-resident.  One warm-up, then --runs turns timed by HIP events on the kernel's stream
(QM_PSB_STAT_LAST_FOLD_US / LAST_EXPECT_US / LAST_EFFLEN_US and the other objects' like).  Every turn's results are held against the
first turn's.  One JSON line."""
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

p = ra.PosBias(mp); s = ra.SeqBias(mp); g = ra.GCBias(mp); f = ra.FragLenDist(mp)
p.add(mp); s.add(mp); g.add(mp); f.add(mp)                               # warm-up
first = p.counts(); sfirst = s.counts()
t_p, t_s, t_g, t_f = [], [], [], []
for _ in range(a.runs):                                                  # (a): in turn, in one process
    p.add(mp); t_p.append(round(p.stat()["last_fold_us"] / 1e3, 3))
    f.add(mp); t_f.append(round(f.stat()["last_fold_us"] / 1e3, 3))
    g.add(mp); t_g.append(round(g.stat()["last_fold_us"] / 1e3, 3))
    s.add(mp); t_s.append(round(s.stat()["last_fold_us"] / 1e3, 3))
st = p.stat()
assert np.array_equal(p.counts(), first * np.uint64(a.runs + 1)), "the observed counts differ from turn to turn"
per = {k: st[k] // (a.runs + 1) for k in ra.PSB_STATS}
single = per["units"] - per["unmapped"] - per["multi"]
gated = per["used"] + per["overhang"]
# the byte floor, as for the GC sweep: all offsets once, one 32-byte sector per single-hit unit, per unit behind the gate txpLen (a
# sector: a gather); no text, no rank structure
floor = (8 * (n + 1) + 32 * single + 32 * gated) / 6.0e12 * 1e3
out.update(psb_sweep_ms=t_p, fld_fold_ms=t_f, gcb_sweep_ms=t_g, sqb_sweep_ms=t_s, stats_per_sweep=per, words_nonzero=int(np.count_nonzero(first)),
           sweep_byte_floor_ms_at_6_0TBps=round(floor, 4))

fc = f.counts() // np.uint64(a.runs + 1)                                 # (b): that run's fragment lengths, a flat first estimate
T = qi.n_txps
L = np.asarray(qi.txp_lens, dtype=np.int64)
q, k = ra.seq_bias_weights(np.ones(T), L, fc)
e0 = p.expect(fc, T, q)                                                  # warm-up
ex = []
for _ in range(a.runs):
    e = p.expect(fc, T, q); ex.append(round(p.stat()["last_expect_us"] / 1e3, 3))
    assert e.tobytes() == e0.tobytes(), "the expected counts differ from turn to turn"
ends = [sum(int(x) for x in e0[end].ravel()) for end in (0, 1)]
assert ends[0] == ends[1], "the two ends differ"
out.update(expect_ms=ex, weight_exponent=k, two_end_sums=ends)

R = ra.pos_bias_ratios(first, e0)                                        # (c): both walks on the same histogram, in turn
se0 = s.expect(fc, T, q)
SR = ra.seq_bias_ratios(sfirst, se0)
v0 = p.eff_lens(fc, T, R); w0 = s.eff_lens(fc, T, SR)                    # warm-up (builds the tile tables)
ef, sf = [], []
for _ in range(a.runs):
    v = p.eff_lens(fc, T, R); ef.append(round(p.stat()["last_efflen_us"] / 1e3, 3))
    w = s.eff_lens(fc, T, SR); sf.append(round(s.stat()["last_efflen_us"] / 1e3, 3))
    assert v.tobytes() == v0.tobytes() and w.tobytes() == w0.tobytes(), "the effective lengths differ from turn to turn"
ls = np.flatnonzero(fc)
pairs = int(sum(int(np.maximum(L - l + 1, 0).sum()) for l in ls))
steps = pairs / 64                                                       # a wavefront step covers 64 starts at one length
out.update(psb_efflen_ms=ef, sqb_efflen_ms=sf, lengths_with_counts=int(ls.size), start_length_pairs=pairs, ratio_min=float(R.min()), ratio_max=float(R.max()),
           lds_read_floor_ms=round(steps * 2 / (256 * 2.4e9) * 1e3, 3), fp64_issue_floor_ms=round(steps * 2 * 4 / (256 * 4 * 2.4e9) * 1e3, 3))
import psb_cases as ps      # noqa: E402
pick = np.linspace(0, T - 1, min(a.sample, T)).astype(np.int64)
t0 = time.time()
vs = ps.eff_lens(L[pick], fc, R)
dt = time.time() - t0
assert vs.tobytes() == v0[pick].tobytes(), "the device's effective lengths differ from the restatement's"
out.update(restatement_sample_txps=int(pick.size), restatement_sample_s=round(dt, 3))
print(json.dumps(out))
