"""The lean kernel's hits-to-mappings pass by itself (qm_lean.inl): the dispatcher the kernels call (lean_h2m), the scalar-indexed loop
(lean_h2m_loop), the 8 x 8 tiles (lean_h2m_tiles) and their single-tile edition, under the lane emulation (tests/emu/qm_emu_h2m.cpp),
against one another and against a plain restatement of the rule (tests/h2m_cases.py, where the cases and the rule live;
test_h2m_tiles_gpu.py runs the same bodies on the device).

Every n from 0 to 64 and every m from 1 to 32 occur; the stashes are seeded random ones built to collide (few transcripts, few positions)
plus the named cases below."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
import h2m_cases as hc  # noqa: E402


@pytest.fixture(scope="module")
def emu():
    import emu_h2m
    emu_h2m._lib()
    return emu_h2m


@pytest.fixture(scope="module")
def h2m_many(emu):
    assert (emu.DISPATCH, emu.LOOP, emu.TILES, emu.ONE_TILE) == (hc.DISPATCH, hc.LOOP, hc.TILES, hc.ONE_TILE)
    return lambda which, cases: [emu.h2m(which, st, m, mi, rc) for st, m, mi, rc in cases]


@pytest.mark.parametrize("n", hc.RANDOM_NS)
def test_random_stashes(h2m_many, n):
    hc.random_stashes(h2m_many, n)


def test_every_interval_count(h2m_many):
    hc.every_interval_count(h2m_many)


@pytest.mark.parametrize("n", hc.SIZES)
def test_one_transcript_fills_the_stash(h2m_many, n):
    hc.one_transcript_fills_the_stash(h2m_many, n)


@pytest.mark.parametrize("n", hc.SIZES)
def test_twice_in_one_interval(h2m_many, n):
    hc.twice_in_one_interval(h2m_many, n)


@pytest.mark.parametrize("n", hc.SIZES)
def test_missing_from_one_interval(h2m_many, n):
    hc.missing_from_one_interval(h2m_many, n)


@pytest.mark.parametrize("n", hc.SIZES)
def test_equal_positions_min_idx_decides(h2m_many, n):
    hc.equal_positions_min_idx_decides(h2m_many, n)


def test_thresholds_of_the_dispatcher(h2m_many, emu):
    hc.thresholds_of_the_dispatcher(h2m_many, emu.tile_range())
