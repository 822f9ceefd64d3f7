"""The ksw2 row kernels ON THE DEVICE: the bodies of the row-kernel tests of test_ksw_variants.py (tests/ksw_rows_cases.py) through the device
probe (tests/device/qm_probe.hip) instead of the lane emulation, against the oracle's qo_ksw_extz2 -- sel_ksw_extz2_rows<32 / 64 / 128 / 1024> and
the eight-per-wavefront register edition as the product compiles them for gfx950, 19 scoring schemes, every target length 1 .. 160, all four
rings, partly filled wavefronts and idle rows.  The alignment blocks live where the product keeps them (LDS, four or eight per wavefront, as
many wavefronts per block as the launch wrapper gives the ring), filled with 0xAB and staged as sel_tasks_align_rows stages them; all the groups
of a scheme are one launch, a group per wavefront.  The 4096-slot ring of the long reads, whose blocks live in device memory, has no emulation
test of its own: it is held to the oracle here."""
import os
import sys

import numpy as np
import pytest

import ksw_rows_cases as kc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "device"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(lib_built, oracle_mod):                                           # (torch opens the device before the probe's runtime does)
    import probe
    probe._lib()
    return probe


def test_the_probe_picks_the_ring_the_launch_wrapper_picks(dev):
    assert [dev.ring_slots(w) for w in (0, 15, 16, 33, 34, 97, 98, 1000, -1)] == [32, 32, 64, 64, 128, 128, 1024, 1024, 1024]


@pytest.mark.parametrize("scheme", kc.SCHEMES)
def test_ksw_rows_kernel_four_at_a_time(dev, scheme):
    before = dev.launches
    kc.four_at_a_time(dev.ksw_rows, scheme)
    assert dev.launches == before + 1                                     # all the groups of the scheme in one launch


@pytest.mark.parametrize("ring", kc.RINGS)
def test_ksw_rows_every_ring_gives_the_same_scores(dev, ring):
    kc.every_ring_gives_the_same_scores(dev.ksw_rows, ring)


@pytest.mark.parametrize("qmax", kc.QMAX)
def test_ksw_rows_longest_alignments(dev, qmax):
    kc.longest_alignments(dev.ksw_rows, qmax)


@pytest.mark.parametrize("w", kc.BANDS_EVERY_TLEN)
def test_ksw_rows_every_target_length(dev, w):
    kc.every_target_length(dev.ksw_rows, w)


@pytest.mark.parametrize("scheme", kc.SAME_SHAPE_SCHEMES)
def test_ksw_rows_same_shape_wavefronts(dev, scheme):
    kc.same_shape_wavefronts(dev.ksw_rows, scheme)


@pytest.mark.parametrize("scheme", kc.EIGHT_SCHEMES)
def test_ksw_rows_eight_per_wavefront(dev, scheme):
    before = dev.launches
    kc.eight_per_wavefront(dev.ksw_rows8, scheme)
    assert dev.launches == before + 1


@pytest.mark.parametrize("w", [15, 98, 1000, -1])
def test_ksw_rows_ring_in_device_memory(dev, w):
    """the 4096-slot ring (blocks in device memory, two wavefronts per block): the same scores as the oracle on the mixed shapes, on
    every target length residue and on the longest alignments a long read produces (2048 bases against targets 20 longer)"""
    scheme = (2, -4, 4, 2, w)
    cases = list(kc.ksw_cases(99, 48))
    groups = [cases[i:i + 4] for i in range(0, len(cases), 4)]
    rng = np.random.default_rng(400 + w)
    for t0 in range(97, 129, 4):
        q = rng.integers(0, 4, 100).astype(np.uint8)
        groups.append([(q, np.resize(q, tlen) ^ (np.arange(tlen) == tlen // 2).astype(np.uint8)) for tlen in range(t0, t0 + 4)][:int(rng.integers(1, 5))])
    long_grp = []
    for qlen in (2048, 2021, 1500):
        q = rng.integers(0, 4, qlen).astype(np.uint8)
        long_grp.append((q, kc.ksw_mutate(rng, q, qlen + 20, sub=0.03, indel=0.01)))
    groups.append(long_grp)
    outs = dev.ksw_rows(groups, scheme, dev.RING_GMEM)
    kc._compare(groups, outs, scheme)
