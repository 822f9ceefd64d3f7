"""The run schedule of the two headline kernels under the lane emulation: duo_wave and lean_wave (the wave bodies qm_duo_kernel and
qm_lean_kernel call) over the adversarial golden pairs with nw = 1, 2 and 5 waves that take runs of R = 1 and 8 neighbouring pairs
(rapmap_amd/csrc/qm_grid.h), held bit for bit to the oracle through mapping_harness.

tests/emu/qm_emu_runs.cpp runs ONE of the two wave drivers over the batch under the schedule asked for and goes on as the library does
behind that kernel: the reads the kernel marked are queued and mapped by the general kernel, stage B merges the pairs that were not merged
in the wavefront, and the pair kernel's own counters are added to stage B's.  A driver that skipped a pair, mapped one twice, or read
another pair's offsets out of a run's staging row would leave hits, offsets or counters that are not the oracle's.

What occurs: 4 234 pairs over 5 waves at R = 8 are 530 runs, 106 for every wave, and the last run holds two pairs (4 234 = 529 x 8 + 2);
the batches of 1, 5 and 7 pairs are shorter than one run (at nw = 2 and 5 the other waves find nothing to do); 9 and 19 pairs are one run
and a short one, two runs and a short one; 8 pairs are exactly one run.  Reads of the golden set have unequal lengths, so offsets are
irregular and reads start at every alignment."""
import pytest

import emu_runs
import mapping_harness as mh
from util import pack

NW = (1, 2, 5)
RUN = (1, 8)
SMALL = (1, 5, 7, 8, 9, 19)
KERNELS = ("pair", "lean")


@pytest.fixture(scope="module")
def golden(synth_small, oracle_mod):
    """the emulation's index, the packed pairs, the oracle's result of the whole set and of its first n pairs for n in SMALL -- computed
    once, never changed"""
    ix, orc, em = mh.emu_of(synth_small["idx"])
    r1, r2 = synth_small["reads1"], synth_small["reads2"]
    assert len(set(len(r) for r in r1)) > 20, "the golden reads are of one length: offsets would be regular"
    batches = {0: pack(r1) + pack(r2)}
    for n in SMALL:
        batches[n] = pack(r1[:n]) + pack(r2[:n])
    want = {n: orc.map_pairs(*a, nthreads=4) for n, a in batches.items()}
    return em, batches, want


@pytest.mark.parametrize("run", RUN)
@pytest.mark.parametrize("nw", NW)
@pytest.mark.parametrize("kernel", KERNELS)
def test_golden_pairs(golden, kernel, nw, run):
    em, batches, want = golden
    a = batches[0]
    n = len(a[1]) - 1
    assert n == 4234 and n % 8 == 2 and (n + 7) // 8 == 530, n          # the last run is short; every wave makes many runs
    er = emu_runs.map_runs(em, kernel, nw, run, *a)
    what = "golden pairs, %s kernel, nw=%d R=%d" % (kernel, nw, run)
    assert er.status == 0, (what, er.status)
    mh.check(want[0], er, what)
    # the kernel itself mapped most of the set, and left the reads it is not built for (N's, IUPAC codes, homopolymer windows ...)
    assert 0 < er.left < n, (what, er.left)
    assert (er.merged > n // 2) if kernel == "pair" else er.merged == 0, (what, er.merged)


@pytest.mark.parametrize("run", RUN)
@pytest.mark.parametrize("nw", NW)
@pytest.mark.parametrize("kernel", KERNELS)
def test_small_batches(golden, kernel, nw, run):
    """batches shorter than a run, of exactly one run, of a run and a short one, of two runs and a short one"""
    em, batches, want = golden
    for n in SMALL:
        er = emu_runs.map_runs(em, kernel, nw, run, *batches[n])
        what = "first %d golden pairs, %s kernel, nw=%d R=%d" % (n, kernel, nw, run)
        assert er.status == 0, (what, er.status)
        mh.check(want[n], er, what)
