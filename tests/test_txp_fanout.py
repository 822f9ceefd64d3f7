"""Families of T transcripts around a shared core (fanout_cases.py: T = 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, plain and diverging),
through the device mapper's source under the lane emulation (tests/emu), against the oracle: bit-exact hits, offsets, counters and
SA-interval lists, and `status == 0` (the emulation's own cross-checks of the pair and lean kernels against the general one).  The same
data runs on the HIP path in test_txp_fanout_gpu.py (-m gpu).

What this reaches: the hits-to-mappings pass of the lean kernel (lean_h2m, qm_lean.inl) and of the pair kernel (qm_duo.inl) on n = T
and n = 2 T entries, at every size where lean_h2m changes its way (the loop, one 8 x 8 tile, several tiles, the loop again), with
transcripts dropped because a narrower second interval does not hold them.  tests/test_h2m_tiles.py holds the pass by itself."""
import pytest

import fanout_cases as fc
import mapping_harness as mh

KERNELS = {"host": {}, "no_pair": {"QM_EMU_NO_DUO": "1"}}


@pytest.fixture(scope="module")
def root(tmp_path_factory, lib_built, oracle_mod):
    return tmp_path_factory.mktemp("txp_fanout")


@pytest.mark.parametrize("kernels", sorted(KERNELS))
@pytest.mark.parametrize("variant", fc.VARIANTS)
@pytest.mark.parametrize("image", ["dense", "ph"])
def test_pairs(root, oracle_mod, image, variant, kernels, monkeypatch):
    """2 x 100 at k = 31; the kernels as the host would run them (the pair kernel first) and without the pair kernel (qm_lean_kernel)"""
    for name, v in KERNELS[kernels].items():
        monkeypatch.setenv(name, v)
    r, er = mh.emu_pairs(fc, root, oracle_mod, 31, 100, image, variant, note=" " + kernels)
    print("%s %s: %d pairs, %d hits, %r" % (r.what, kernels, r.n, len(r.res.hits), r.res.counters))
    assert r.n <= 400, r.n


def test_the_data_reaches_every_size(root, oracle_mod):
    """asked of the oracle alone: reads with one interval of every T, and reads with two intervals of which the second is the narrower"""
    r = mh.emu_ref(fc, root, oracle_mod, 31, 100, "dense", "default")
    one, two = fc.reach(r.res)
    print("fan-out, %s: single intervals of %r suffixes; (wider, narrower) pairs %r" % (r.what, sorted(one), sorted(two)))
    assert set(fc.SIZES) <= one, sorted(one)
    assert {T for (T, t) in two} >= {T for T in fc.SIZES if T >= 7}, sorted(two)


def test_what_the_pair_and_lean_kernels_leave(root, oracle_mod, capfd, monkeypatch):
    """two intervals of 33 suffixes do not fit the lean kernel's stash of 64: such reads are left to the general kernel, and only a few others"""
    import kmer_cases as kc
    r = mh.emu_ref(fc, root, oracle_mod, 31, 100, "dense", "default")
    monkeypatch.setenv("QM_EMU_LEAN_STATS", "1")
    capfd.readouterr()
    er = mh.emu_of(r.idx)[2].map(*r.a)
    left = kc.emu_left(capfd.readouterr().err)
    print("fan-out, %s: of %d reads the emulation's pair / lean kernels left %r" % (r.what, 2 * r.n, left))
    assert er.status == 0
    assert 0 < left["lean"] < r.n // 4 and 0 < left["pair"] < r.n, left
