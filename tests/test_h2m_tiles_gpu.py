"""The lean kernel's hits-to-mappings pass by itself ON THE DEVICE: the bodies of test_h2m_tiles.py (tests/h2m_cases.py) through the device probe
(tests/device/qm_probe.hip) instead of the lane emulation -- lean_h2m, lean_h2m_loop, lean_h2m_tiles<false> and <true> as the product compiles
them for gfx950, every n from 0 to 64 and every m from 1 to 32, against the same plain restatement of the rule.  A test is one launch per
edition: one stash per wavefront, four different stashes per block of 256 threads, each in its wavefront's LDS with 0xA5 in the unused slots."""
import os
import sys

import pytest

import h2m_cases as hc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "device"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(lib_built):                                                       # (torch opens the device before the probe's runtime does)
    import probe
    probe._lib()
    assert (probe.DISPATCH, probe.LOOP, probe.TILES, probe.ONE_TILE) == (hc.DISPATCH, hc.LOOP, hc.TILES, hc.ONE_TILE)
    return probe


@pytest.fixture
def h2m_many(dev):
    """the probe's callable; afterwards: the test made one launch per edition at the most"""
    before = dev.launches
    yield dev.h2m_many
    assert 1 <= dev.launches - before <= len(hc.EDITIONS)


def test_the_dispatcher_changes_edition_where_the_emulation_does(dev):
    import emu_h2m
    assert dev.tile_range() == emu_h2m.tile_range()


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


def test_thresholds_of_the_dispatcher(h2m_many, dev):
    hc.thresholds_of_the_dispatcher(h2m_many, dev.tile_range())
