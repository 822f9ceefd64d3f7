"""The -s question scorer and the strip alignments BY THEMSELVES ON THE DEVICE: the questions of tests/sel_side_cases.py through the device probe
(tests/device/qm_probe.hip: qp_sel_side, qp_sel_strip) -- sel_side_score<G> with the product's own group reductions SelRed2 / 4 / 8 / 16, launched
as qm_sel_score_kernel launches it (256-thread blocks, 256 / G questions per block, a question count that is no multiple of that: the last groups
sit beside idle lanes), and sel_tasks_strip on __shared__ StripMem[4], four tasks per wavefront -- against classify(), the oracle's qo_ksw_extz2
and, bit for bit, the lane emulation (tests/emu/qm_emu_sel.cpp).  All questions of a scheme are one launch per G."""
import collections
import os
import sys

import numpy as np
import pytest

import sel_side_cases as sc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "device"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

pytestmark = pytest.mark.gpu
LANES = (2, 4, 8, 16)


@pytest.fixture(scope="module")
def dev(lib_built, oracle_mod):                                           # (torch opens the device before the probe's runtime does)
    import probe
    probe._lib()
    return probe


def test_the_probe_and_the_cases_agree_on_the_longest_strip_read(dev):
    assert dev._lib().qp_sel_max_read_len() == sc.MAX_READ_LEN


@pytest.mark.parametrize("scheme", sc.SCHEMES)
def test_sel_side_score_and_strip_on_the_device(dev, scheme):
    """per G: the class is classify()'s, the queued tasks carry the restated geometry, known / ungapped scores are the reference's, the keys follow
    the target windows, and key, kind, tsc and the task records are the emulation's bit for bit; then the strip alignments of the scheme in one
    launch, four per wavefront with the last wavefront partly filled: every score is qo_ksw_extz2's and the emulation's"""
    import emu_sel
    cs = sc.cases(scheme)
    n = sc.check_floors(cs)                                               # (on classify() alone, before anything runs)
    assert len(cs.batch) % 128 and (n["strip"] % 4 or not n["strip"]), (len(cs.batch), n)     # the last groups / the last wavefront partly filled
    ekind, etsc0, ekey, etask, _ = emu_sel.sel_side(cs.batch, 0, scheme, strip=False)
    _, etsc, _, _, enstrip = emu_sel.sel_side(cs.batch, 0, scheme, strip=True)
    before = dev.launches
    for G in LANES:
        kind, tsc, key, task = dev.sel_side(G, cs.batch, 0, scheme)
        sc.check_classes(cs, kind)
        sc.check_tasks(cs, task)
        sc.check_scores(cs, tsc, False)
        sc.check_keys(cs, kind, key)
        for name, got, want in (("kind", kind, ekind), ("tsc", tsc, etsc0), ("key", key, ekey), ("task", task, etask)):
            diff = np.nonzero((got != want).reshape(len(kind), -1).any(axis=1))[0]
            assert not len(diff), "%d lanes per question: %s differs from the emulation's at %d questions, first %r" % (G, name, len(diff), diff[:5].tolist())
    assert dev.launches == before + len(LANES)                            # all the questions of the scheme in one launch per G
    strip = np.nonzero(kind & 4)[0]
    assert len(strip) == enstrip == n["strip"]
    if len(strip):
        out = dev.sel_strip(task[strip], cs.batch, scheme)
        assert dev.launches == before + len(LANES) + 1
        tsc = tsc.copy(); tsc[strip] = out
        sc.check_scores(cs, tsc, True)
        assert np.array_equal(tsc, etsc), "strip scores differ from the emulation's at %r" % np.nonzero(tsc != etsc)[0][:5].tolist()


@pytest.mark.parametrize("policy", [1, 2])
def test_bowtie2_policies_drop_overhanging_positions(dev, policy):
    """alnPolicy 1 / 2 on the device: positions before a transcript's start and reads that reach its end get the lowest score, no key, no task"""
    import emu_sel
    scheme = sc.SCHEMES[0]
    cs = sc.cases(scheme, policy)
    assert collections.Counter(cs.cls)["dropped"] >= 100
    ekind, etsc0, ekey, etask, _ = emu_sel.sel_side(cs.batch, policy, scheme, strip=False)
    for G in LANES:
        kind, tsc, key, task = dev.sel_side(G, cs.batch, policy, scheme)
        sc.check_classes(cs, kind)
        sc.check_tasks(cs, task)
        sc.check_scores(cs, tsc, False)
        assert np.array_equal(kind, ekind) and np.array_equal(tsc, etsc0) and np.array_equal(key, ekey) and np.array_equal(task, etask)
