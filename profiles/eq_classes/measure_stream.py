"""FASTQ -> classes through the stream without hits (QM_STREAM_EQ_CLASSES | QM_STREAM_NO_HITS) against FASTQ -> hits, same files.

    python profiles/eq_classes/measure_stream.py [--root TREE] --mode hits|classes --fq1 F1 --fq2 F2 [--write PAIRS]

--write PAIRS: first write PAIRS simulated pairs of the headline workload to F1 / F2 (once; the runs then share the files).
--root: the tree to import from -- the parent commit's for the `hits` side of the comparison.  One JSON line."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ap.add_argument("--mode", default="hits")
ap.add_argument("--fq1", required=True); ap.add_argument("--fq2", required=True)
ap.add_argument("--write", type=int, default=0)
ap.add_argument("--genes", type=int, default=40000)
ap.add_argument("--threads", type=int, default=16)
a = ap.parse_args()
sys.path.insert(0, a.root)
sys.argv = sys.argv[:1]

import numpy as np          # noqa: E402
import torch                # noqa: E402
import bench                # noqa: E402
import rapmap_amd as ra     # noqa: E402

idx = bench.build_or_reuse_index(a.genes, 42, 31, 0, 1, bench.default_cache())
qi = ra.QuasiIndex(idx)
if a.write:
    dev = torch.device("cuda:0")
    text, starts, lens = bench.load_text_to_gpu(qi, dev)
    s1, s2, off = bench.make_reads_gpu(text, starts, lens, a.write, 43, dev)
    for fn, s in ((a.fq1, s1), (a.fq2, s2)):
        r = s[: a.write * 100].cpu().numpy().reshape(a.write, 100)
        rec = np.full((a.write, 214), ord("I"), dtype=np.uint8)           # @xxxxxxxx\n read \n+\n quality \n
        rec[:, 0] = ord("@"); rec[:, 1:9] = np.frombuffer(b"".join(b"%08d" % i for i in range(a.write)), dtype=np.uint8).reshape(a.write, 8)
        rec[:, 9] = 10; rec[:, 10:110] = r; rec[:, 110] = 10; rec[:, 111] = ord("+"); rec[:, 112] = 10; rec[:, 213] = 10
        rec.tofile(fn)
    del s1, s2, text
ra.reserve_stream_memory(1280 << 20)
keep = ra.QuasiMapper(qi, 0)                                               # the replica stays; the stream's contexts share it
t0 = time.perf_counter()
kw = dict(eq_classes=True, hits=False) if a.mode == "classes" else {}
st = ra.MappedStream(qi, a.fq1, a.fq2, batch_units=1 << 18, threads=a.threads, names=False, **kw)
units = hits = 0
for b in st:
    units += b.n; hits += b.n_hits
out = {"root": os.path.relpath(a.root), "mode": a.mode, "pairs": units, "n_hits": hits}
if a.mode == "classes":
    o, t, c = st.eq_classes()
    out.update(n_classes=len(c), total=int(c.sum()))
out["seconds"] = round(time.perf_counter() - t0, 4)
out["M_pairs_per_s"] = round(units / out["seconds"] / 1e6, 2)
st.close()
print(json.dumps(out))
