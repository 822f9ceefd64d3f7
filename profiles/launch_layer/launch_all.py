"""profiles/launch_layer/launch_all.py -- fixed synthetic batches of a few thousand units on a 60-gene index, chosen so that every launcher
of the kernel launch layer (rapmap_amd/csrc/qm_device.h) runs at least once.  Run under `rocprofv3 --kernel-trace` (the program after
`--`, nothing else traced), once with the parent commit's library (QM_LIB_OVERRIDE) and once with this tree's; kernel_grids.py turns each
trace into the sorted multiset of (kernel, grid, workgroup) and the two must be equal: profiles/launch_layer/results/kernel_grids.txt.

Prints one line per case with a digest of what the call returned, so that the two runs' results can be compared too."""
import hashlib
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def say(case, r):
    if hasattr(r, "hits"):
        print("%-44s hits %8d  %s  %s" % (case, r.n_hits, digest(r.hit_offsets, r.hits), sorted(r.counters.items())), flush=True)
    else:
        print("%-44s %s" % (case, digest(*r)), flush=True)


class env:
    """os.environ with a few variables set for the calls inside (the library reads these per call)"""
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def main():
    import torch
    torch.cuda.init()                                            # (torch's HIP runtime opens the device before the library's)
    import rapmap_amd as ra
    from rapmap_amd import synth
    names, txps = synth.make_transcriptome(60, seed=3)
    n = 4000
    r100 = synth.make_reads(txps, n, seed=4)
    r150 = synth.make_reads(txps, n, seed=5, read_len=150)
    r300 = synth.make_reads(txps, n // 2, seed=6, read_len=300)
    rN = synth.make_reads(txps, n, seed=7, n_rate=0.004)         # about a third of the reads carry an N
    # single-end: 3 000 reads of 100 characters and 24 of 600 (the long-read pass)
    r600 = synth.make_reads(txps, 24, seed=8, read_len=600)
    mixed = [bytes(r100[0][i * 100:(i + 1) * 100]) for i in range(3000)]
    for i in range(24):
        mixed.insert(100 * i + 7, bytes(r600[0][i * 600:(i + 1) * 600]))
    mseq, moff = ra.pack_reads(mixed)
    sel, nosens = ra.default_opts(sel_aln=1), ra.default_opts(sensitive=0)
    with tempfile.TemporaryDirectory() as td:
        fa = os.path.join(td, "t.fa")
        synth.write_fasta(fa, names, txps)
        dense, ph = os.path.join(td, "idx"), os.path.join(td, "idx_ph")
        ra.build_index(fa, dense, threads=4)
        ra.build_index(fa, ph, threads=4, perfect_hash=True)
        qi = ra.QuasiIndex(dense)
        mp = ra.QuasiMapper(qi, 0)
        s1, s2, off, _ = r100
        say("2x100", mp.map_pairs(s1, off, s2, off))
        pad = np.zeros(8, np.uint8)
        dv = [torch.from_numpy(x).cuda() for x in (np.concatenate([s1, pad]), off, np.concatenate([s2, pad]), off)]
        torch.cuda.synchronize()
        with env(QM_SPLIT_MIN="1000"):                           # two parts: the lean kernel on one, the pair kernel on the other
            say("2x100 resident, two parts", mp.map_device(n, dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), 100, fetch=True))
        say("single-end 100", mp.map_reads(s1, off))
        say("2x150", mp.map_pairs(r150[0], r150[2], r150[1], r150[2]))
        say("2x300", mp.map_pairs(r300[0], r300[2], r300[1], r300[2]))
        say("single-end 100 + 24 x 600", mp.map_reads(mseq, moff))
        say("2x100 --noSensitive", mp.map_pairs(s1, off, s2, off, opts=nosens))
        say("2x300 --noSensitive", mp.map_pairs(r300[0], r300[2], r300[1], r300[2], opts=nosens))
        say("2x100 -s", mp.map_pairs(s1, off, s2, off, opts=sel))
        with env(QM_SEL_PACK="0"):
            say("2x100 -s QM_SEL_PACK=0", mp.map_pairs(s1, off, s2, off, opts=sel))
        say("2x150 -s", mp.map_pairs(r150[0], r150[2], r150[1], r150[2], opts=sel))
        say("2x300 -s", mp.map_pairs(r300[0], r300[2], r300[1], r300[2], opts=sel))
        say("single-end 100 + 24 x 600 -s", mp.map_reads(mseq, moff, opts=sel))
        found, ioff, ints = mp.collect_reads(mseq, moff)
        say("collect_reads (100 + 24 x 600)", (found, ioff, ints))
        say("hits_to_mappings", mp.hits_to_mappings(np.diff(moff).astype(np.int32), ioff, ints))
        with env(QM_NPASS_MIN="1"):                              # the N-aware edition of the lean kernel over what the first pass left
            say("2x100 with N, QM_NPASS_MIN=1", mp.map_pairs(rN[0], rN[2], rN[1], rN[2]))
            say("2x100 with N -s, QM_NPASS_MIN=1", mp.map_pairs(rN[0], rN[2], rN[1], rN[2], opts=sel))
            print("%-44s %d" % ("  reads the N-aware pass mapped", mp.stat(ra.api.QM_STAT_N_PASS_READS)), flush=True)
        mp.close(); qi.close()
        qp = ra.QuasiIndex(ph)
        mp = ra.QuasiMapper(qp, 0, ph_compact=True)              # the compact -p image
        say("-p compact 2x100", mp.map_pairs(s1, off, s2, off))
        say("-p compact single-end 100 + 24 x 600", mp.map_reads(mseq, moff))
        say("-p compact 2x150", mp.map_pairs(r150[0], r150[2], r150[1], r150[2]))
        say("-p compact 2x100 --noSensitive", mp.map_pairs(s1, off, s2, off, opts=nosens))
        say("-p compact 2x100 -s", mp.map_pairs(s1, off, s2, off, opts=sel))
        mp.close(); qp.close()
    print("launch_all done", flush=True)


if __name__ == "__main__":
    main()
