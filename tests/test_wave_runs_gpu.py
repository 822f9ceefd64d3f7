"""Runs of neighbouring pairs per wavefront on the HIP path (libqmap_mi355.so through its C ABI), against the oracle.

The two headline kernels hand a wavefront runs of R neighbouring pairs (rapmap_amd/csrc/qm_grid.h) and stage a run's offsets in LDS once;
R is 8 for a batch that has 8 runs' worth of pairs for every wavefront that can be resident, and shrinks below that.  Here the synth_small
index and its adversarial pairs (reads of unequal lengths: irregular offsets, reads that start at every alignment) go through the pair
kernel and through qm_lean_kernel (mapping_harness.headline, debug=False):

  * the first 1, 7, 8, 9 and 19 pairs, and the whole set (4 234 pairs): R = 1 on any device with more than 16 compute units;
  * the set tiled (tile_cases.tile: shuffled copies, held to tile_cases.expected of the oracle's result) until the batch has R = 8 --
    under the default grid every wavefront then makes at most one run; under the smallest grid (QM_BLOCKS_PER_CU=1 QM_GRID_OVERSUB=1
    QM_DUO_OVERSUB=1, four wavefronts per compute unit) the copies are chosen so that every wavefront makes three runs and more, the last
    run of the batch is short, and the offsets' two staging rows are each used again.  The grid knobs are read once per process, so that
    leg runs in a fresh child process: this file as a script;
  * the whole set with QM_NPASS_MIN=1, so that qm_lean_kernel's N-aware edition goes over the reads the first pass left (it shares the
    wave driver and keeps a request per iteration), and 150-character pairs through the wide edition (one read per wavefront).

Hits, offsets and the six counters are bit-identical to the oracle's.  No error path is provoked here."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [HERE, os.path.join(HERE, "emu"), os.path.dirname(HERE)]

import mapping_harness as mh
import tile_cases as tc
from util import pack

pytestmark = pytest.mark.gpu

SMALL = (1, 7, 8, 9, 19)
RUN = 8                      # qm_grid.h, WAVE_RUN_DEFAULT
SEED = 20261


def golden_reads():
    import samfmt as sam
    gold = os.path.join(HERE, "golden", "synth_small")
    r1 = sam.read_fastq(os.path.join(gold, "reads_1.fastq.gz"))[1]
    r2 = sam.read_fastq(os.path.join(gold, "reads_2.fastq.gz"))[1]
    assert len(r1) == len(r2) == 4234 and len(set(len(r) for r in r1)) > 20, "the golden reads are not the ragged set this test is about"
    return r1, r2


def wide_reads(fasta):
    """600 pairs of 150 characters from the synth_small transcripts (test_emu_parity.test_long_reads_ns4 draws its reads the same way)"""
    from rapmap_amd import synth
    txt = open(fasta).read().split("\n")
    txps = [np.frombuffer(l.upper().encode(), dtype=np.uint8) for l in txt if l and l[0] != ">"][:300]
    txps = [t for t in txps if t.size >= 600 and not (t == ord("N")).any()]
    s1, s2, off, _ = synth.make_reads(txps, 600, seed=6, read_len=150, err=0.02)
    return s1, off, s2, off


def copies_for(n, num_cu, smallest):
    """copies of n pairs that give the batch R = 8: RUN pairs for each of the num_cu x 32 wavefronts that can be resident -- under the
    smallest grid num_cu x 4, and three runs for each of them"""
    need = RUN * num_cu * 4 * 3 if smallest else RUN * num_cu * 32
    copies = -(-(need + RUN) // n)
    while (copies * n) % RUN == 0:                             # ... and a last run that is short
        copies += 1
    return copies


def run_legs(idx, fasta, num_cu, smallest):
    """every leg of the module under this process's grid knobs -> the lines to print"""
    import rapmap_amd as ra
    orc = mh.oracle_of(idx)[1]
    r1, r2 = golden_reads()
    whole = pack(r1) + pack(r2)
    n = len(r1)
    want_whole = orc.map_pairs(*whole, nthreads=8)
    smalls = []
    for m in SMALL:
        a = pack(r1[:m]) + pack(r2[:m])
        smalls.append((m, a, orc.map_pairs(*a, nthreads=2)))
    copies = copies_for(n, num_cu, smallest)
    tiled, perm = tc.tile(whole, copies, SEED)
    want_tiled = tc.expected(want_whole, perm, copies)
    units = copies * n
    assert units < tc.MAX_UNITS, "%d copies of %d pairs are %d: not one launch on %d compute units" % (copies, n, units, num_cu)
    waves = num_cu * 4 if smallest else num_cu * 32
    assert units >= RUN * waves * (3 if smallest else 1) and units % RUN != 0, (units, waves)    # R = 8; the batch's last run is short
    lines = []
    stat = lambda mp, k: mp.stat(getattr(ra, "QM_STAT_" + k))
    for kernel in mh.HEADLINE_KERNELS:
        t0 = time.perf_counter()
        with mh.headline(idx, kernel) as (qi, mp):
            for m, a, want in smalls:
                mh.check(want, mp.map_pairs(*a), "%s kernel, first %d pairs" % (kernel, m))
                assert stat(mp, "LEAN_READS") == 2 * m, (kernel, m, stat(mp, "LEAN_READS"))
            mh.check(want_whole, mp.map_pairs(*whole), "%s kernel, %d pairs" % (kernel, n))
            mh.check_headline(mp, kernel, n)
            mh.check(want_tiled, mp.map_pairs(*tiled), "%s kernel, %d copies of %d pairs" % (kernel, copies, n))
            mh.check_headline(mp, kernel, units)
            assert stat(mp, "RELAUNCHES") == 0, stat(mp, "RELAUNCHES")
            os.environ["QM_NPASS_MIN"] = "1"                  # (read per call)
            try:
                mh.check(want_whole, mp.map_pairs(*whole), "%s kernel and the N-aware pass, %d pairs" % (kernel, n))
                npass = stat(mp, "N_PASS_READS")
                assert npass > 0, "the N-aware pass mapped nothing: %d" % npass
            finally:
                del os.environ["QM_NPASS_MIN"]
        lines.append("%s kernel%s: %d, %s and %d pairs; %d copies = %d pairs in runs of %d over %d wavefronts (%d runs each at least); N-aware pass %d reads; %.2f s"
                     % (kernel, ", smallest grid" if smallest else "", SMALL[0], ", ".join(str(m) for m in SMALL[1:]), n, copies, units, RUN, waves,
                        units // (RUN * waves), npass, time.perf_counter() - t0))
    t0 = time.perf_counter()
    wa = wide_reads(fasta)
    want_wide = orc.map_pairs(*wa, nthreads=8)
    with mh.gpu_mapper(idx, debug=False, pair_kernel=False, wide_reads=True) as (qi, mp):
        mh.check(want_wide, mp.map_pairs(*wa), "wide lean kernel, 600 pairs of 150")
        assert stat(mp, "LEAN_READS") == 2 * 600, "the wide lean kernel did not run: QM_STAT_LEAN_READS %d" % stat(mp, "LEAN_READS")
    lines.append("wide lean kernel%s: 600 pairs of 150 characters; %.2f s" % (", smallest grid" if smallest else "", time.perf_counter() - t0))
    return lines


@pytest.fixture(scope="module")
def num_cu(lib_built):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_default_grid(synth_small, oracle_mod, num_cu):
    bad = [k for k in tc.GRID_KNOBS + ("QM_WAVE_RUN",) if k in os.environ]
    assert not bad, "a grid knob is set in this process: %r" % bad
    for line in run_legs(synth_small["idx"], synth_small["fasta"], num_cu, smallest=False):
        print(line)


def test_smallest_grid(synth_small, oracle_mod, num_cu):
    """QM_BLOCKS_PER_CU=1 QM_GRID_OVERSUB=1 QM_DUO_OVERSUB=1 in a fresh process: every wavefront makes three runs of eight and more"""
    e = {k: v for k, v in os.environ.items() if k not in tc.GRID_KNOBS + ("QM_WAVE_RUN",)}
    e.update(tc.SMALLEST_GRID)
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, os.path.abspath(__file__), synth_small["idx"], synth_small["fasta"]], env=e, capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:])
    print("the child process: %.2f s" % (time.perf_counter() - t0))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "wave runs ok" in p.stdout.splitlines()[-1]


def _child(idx, fasta):
    import torch
    torch.cuda.init()                                            # (torch's HIP runtime opens the device before the library's: conftest.lib_built)
    from oracle import oracle
    oracle.build()
    assert all(os.environ.get(k) == v for k, v in tc.SMALLEST_GRID.items()), "the grid knobs are not set"
    for line in run_legs(idx, fasta, torch.cuda.get_device_properties(0).multi_processor_count, smallest=True):
        print(line)
    print("wave runs ok")


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
