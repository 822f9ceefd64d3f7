"""profiles/tally_frame/rank_build.py -- what QM_GCB_STAT_RANK_BUILD_US holds besides the build of the GC rank structure.

    python profiles/tally_frame/rank_build.py cold|warm

The structure is built by the first GCBias of a process on an index replica, between two HIP events on the object's stream.  The
build's kernels (gcb_mask_wave, gcb_rank_wave) are instantiated in the same code object as every other wave body and sweep of the
estimation objects, and the runtime loads a code object at the first launch out of it.  `cold`: as profiles/gcb/measure_gcb.py does it,
the GCBias is the first estimation object of the process, so that load falls between the two events.  `warm`: an EqClasses folds the
batch first -- its wave bodies come from the same code object in every version of the library --, so the load has happened before the
first event.  bench.py's config-2 index, a small batch.  One JSON line: {"mode": ..., "rank_build_ms": ...}."""
import json
import os
import sys

mode = sys.argv[1]
assert mode in ("cold", "warm")
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.argv = sys.argv[:1]

import torch                # noqa: E402
import bench                # noqa: E402
import rapmap_amd as ra     # noqa: E402

dev = torch.device("cuda:0")
qi = ra.QuasiIndex(bench.build_or_reuse_index(40000, 42, 31, 0, 1, bench.default_cache()))
mp = ra.QuasiMapper(qi, 0)
text, starts, lens = bench.load_text_to_gpu(qi, dev)
n = 100_000
s1, s2, off = bench.make_reads_gpu(text, starts, lens, n, 43, dev)
torch.cuda.synchronize()
mp.map_device(n, s1.data_ptr(), off.data_ptr(), s2.data_ptr(), off.data_ptr(), 100, fetch=False)
if mode == "warm":
    t = ra.EqClasses(mp)
    t.add(mp)
    t.close()
g = ra.GCBias(mp)
print(json.dumps({"mode": mode, "rank_build_ms": g.stat()["rank_build_us"] / 1e3}))
g.close(); mp.close(); qi.close()
