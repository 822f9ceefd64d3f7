"""The -s question scorer and the strip alignments BY THEMSELVES, through the lane emulation (tests/emu/qm_emu_sel.cpp): sel_side_score<1> with
SelRedOne and sel_tasks_strip of rapmap_amd/csrc/qm_sel.inl on the questions of tests/sel_side_cases.py -- every read length at the edges of the
8-character words, both orientations, positions at both ends of a transcript, substitutions on and beside the word boundaries, a neighbouring
diagonal that turns clean exactly at, before and behind the rule's threshold, N / lower case / bytes below 4, reads packed back to back --
against classify() (who answers) and the oracle's qo_ksw_extz2 (what the answer is).  test_sel_side_gpu.py runs the same on the device with
2, 4, 8 and 16 lanes per question."""
import collections
import functools
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.join(HERE, "emu"))
import emu_sel  # noqa: E402
import sel_side_cases as sc  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_mod):
    return oracle_mod


@functools.lru_cache(maxsize=None)
def scored(scheme, policy=0):
    """the scheme's questions, the floors on classify() alone, then the code under test"""
    cs = sc.cases(scheme, policy)
    if policy == 0:
        sc.check_floors(cs)
    return (cs,) + emu_sel.sel_side(cs.batch, policy, scheme)


def test_the_cases_know_the_longest_strip_read():
    assert emu_sel.max_read_len() == sc.MAX_READ_LEN


@pytest.mark.parametrize("scheme", sc.SCHEMES)
def test_floors_no_class_is_left_out(scheme):
    """per scheme, on classify() alone: at least 500 known, 300 strip and 100 ksw2 questions where the scheme's limits admit the class, and at
    least 100 questions that a one-gap path wins on each diagonal rule 2 admits"""
    n = sc.check_floors(sc.cases(scheme))
    print(scheme, dict(n))


@pytest.mark.parametrize("scheme", sc.SCHEMES)
def test_the_class_is_classifys(scheme):
    cs, kind, tsc, key, task, nstrip = scored(scheme)
    sc.check_classes(cs, kind)
    assert nstrip == collections.Counter(cs.cls)["strip"]


@pytest.mark.parametrize("scheme", sc.SCHEMES)
def test_queued_tasks_carry_the_restated_geometry(scheme):
    cs, kind, tsc, key, task, nstrip = scored(scheme)
    sc.check_tasks(cs, task)


@pytest.mark.parametrize("scheme", sc.SCHEMES)
def test_scores_are_the_oracles(scheme):
    """known and strip == qo_ksw_extz2, ungapped == the plain count, dropped / off_end / waiting for ksw2 == the lowest score"""
    cs, kind, tsc, key, task, nstrip = scored(scheme)
    sc.check_scores(cs, tsc, True)


@pytest.mark.parametrize("scheme", sc.SCHEMES)
def test_keys_follow_the_target_window(scheme):
    cs, kind, tsc, key, task, nstrip = scored(scheme)
    sc.check_keys(cs, kind, key)


@pytest.mark.parametrize("policy", [1, 2])
@pytest.mark.parametrize("scheme", sc.SCHEMES[:4])
def test_bowtie2_policies_drop_overhanging_positions(scheme, policy):
    """alnPolicy 1 / 2: a position before the transcript's start or a read that reaches its end gets the lowest score, no key and no task; every
    other question is answered as under the default policy"""
    cs, kind, tsc, key, task, nstrip = scored(scheme, policy)
    n = collections.Counter(cs.cls)
    assert n["dropped"] >= 100 and len(cs.cls) >= 2 * n["dropped"], n
    sc.check_classes(cs, kind)
    sc.check_tasks(cs, task)
    sc.check_scores(cs, tsc, True)
