"""The device mapper's source under the lane emulation (tests/emu) at k-mer lengths other than 31, against the oracle: bit-exact hits,
offsets, counters and SA-interval lists, and `status == 0` (the emulation's own cross-checks of the pair, lean and packed kernels against
the general one).  The same cases run on the HIP path in test_kmer_lengths_gpu.py (-m gpu); data and checks are in kmer_cases.py.

The reference is the oracle, which reads k from the index header: the reference's own binary cannot be built here, so there is no
golden SAM at another k.  test_error_free_pairs_* is the one check that does not go through the oracle."""
import pytest

import emu
import kmer_cases as kc
import mapping_harness as mh
from util import pack


@pytest.fixture(scope="module")
def root(tmp_path_factory, lib_built, oracle_mod):
    return tmp_path_factory.mktemp("kmer_lengths")


def _run(idx, oracle_mod, q1, o1, q2, o2, variant, what, ns=2, ints=True):
    """one paired call through the oracle and the emulation"""
    ix, orc, em = mh.emu_of(idx)
    oopts, eopts = mh.opts_for(variant, oracle_mod, emu.default_opts)
    ints = ints and variant != "selAln"
    res = orc.map_pairs(q1, o1, q2, o2, opts=oopts, nthreads=4, want_ints=ints)
    er = em.map(q1, o1, q2, o2, opts=eopts, ns=ns)
    assert er.status == 0, (what, er.status)
    mh.check_emu(res, er, what, ints=ints)
    return res, er


def _run_single(idx, oracle_mod, reads, variant, what, ns=2):
    ix, orc, em = mh.emu_of(idx)
    oopts, eopts = mh.opts_for(variant, oracle_mod, emu.default_opts)
    q, o = pack(reads)
    assert (len(o) - 1) % 2 == 1
    res = orc.map_single(q, o, opts=oopts, nthreads=4)
    er = em.map(q, o, opts=eopts, ns=ns)
    assert er.status == 0, (what, er.status)
    mh.check(res, er, what)
    return res, er


def _golden(root, oracle_mod, k, image, variant, capfd, monkeypatch):
    idx = kc.index_for(root, k, image)
    q1, o1, q2, o2 = kc.golden_reads()[4]
    if variant == "default":
        monkeypatch.setenv("QM_EMU_LEAN_STATS", "1")
        capfd.readouterr()
    res, er = _run(idx, oracle_mod, q1, o1, q2, o2, variant, "golden reads, k=%d %s %s" % (k, image, variant))
    assert res.counters["peHits"] > 1000
    if variant == "default":
        left = kc.emu_left(capfd.readouterr().err)
        print("k=%d %s: the emulation's pair / lean kernels left %s" % (k, image, left))
        assert {"pair": left["pair"], "lean": left["lean_first_pass"]} == kc.EXPECT_LEFT[(k, image)], (k, image, left)
        return left, 2 * (len(o1) - 1)


@pytest.mark.parametrize("image", ["dense", "ph"])
@pytest.mark.parametrize("variant", sorted(mh.PLAIN_SETS))
def test_golden_reads_k21(root, oracle_mod, variant, image, capfd, monkeypatch):
    """synth_small's adversarial pairs at k = 21, every option variant of test_emu_parity, dense and -p"""
    _golden(root, oracle_mod, 21, image, variant, capfd, monkeypatch)


@pytest.mark.parametrize("image", ["dense", "ph"])
@pytest.mark.parametrize("variant", sorted(kc.SOME))
@pytest.mark.parametrize("k", [15, 17, 29])
def test_golden_reads_other_k(root, oracle_mod, k, variant, image, capfd, monkeypatch):
    _golden(root, oracle_mod, k, image, variant, capfd, monkeypatch)


def test_golden_reads_k9_nearly_everything_is_left(root, oracle_mod, capfd, monkeypatch):
    """k = 9: 4 * popc + 6 >= 9 holds with one lane of four equal characters, so the pair and lean kernels leave nearly every read to the
    general kernel -- the regime is what is tested: they must leave them, and what they take must still be right"""
    left, nreads = _golden(root, oracle_mod, kc.K_SMALL, "dense", "default", capfd, monkeypatch)
    assert 0 < nreads - left["lean"] < nreads // 4, left
    assert 0 < nreads - left["pair"] < nreads // 4, left


@pytest.mark.parametrize("variant", sorted(kc.FEW))
@pytest.mark.parametrize("k", kc.KS)
def test_edge_reads(root, oracle_mod, k, variant):
    """mates of length k - 1 .. k + 2, 2 k - 1 .. 2 k + 1 and around the 64- and 128-character slots, with an N at k, k - 1, L - k - 1, a run
    of k + 2 equal bases, a `$`, ...: paired, and single-end with an odd count"""
    idx = kc.index_for(root, k, "dense")
    r1, r2 = kc.edge_reads(idx, k)
    q1, o1 = pack(r1); q2, o2 = pack(r2)
    res, er = _run(idx, oracle_mod, q1, o1, q2, o2, variant, "edge reads, k=%d %s" % (k, variant))
    assert res.counters["peHits"] > len(r1) // 4
    _run_single(idx, oracle_mod, mh.odd_single(r1, r2), variant, "edge reads single-end, k=%d %s" % (k, variant))


@pytest.mark.parametrize("variant", sorted(kc.FEW))
@pytest.mark.parametrize("k", kc.KS)
def test_run_reads(root, oracle_mod, k, variant, capfd, monkeypatch):
    """homopolymer runs of k - 7 .. k + 9 at every alignment of the four-characters-per-lane packing: the pair / lean kernels' rule
    4 * popc + 6 >= k against isHomoPolymer(k)"""
    rd = kc.run_reads(root, k)
    r1, r2 = rd["reads1"], rd["reads2"]
    q1, o1 = pack(r1); q2, o2 = pack(r2)
    if variant == "default":
        monkeypatch.setenv("QM_EMU_LEAN_STATS", "1")
        capfd.readouterr()
    res, er = _run(rd["idx"], oracle_mod, q1, o1, q2, o2, variant, "run reads, k=%d %s" % (k, variant))
    assert res.counters["peHits"] > len(r1) // 4
    if variant == "default":
        # the reads fall on both sides of the rule: more are left than truly hold a window of k equal bases or an N (every one of
        # those is), and reads with a shorter run are taken
        left = kc.emu_left(capfd.readouterr().err)
        windows = sum(kc.has_window(r, k) or b"N" in r for r in r1 + r2)
        print("k=%d: %d reads, %d hold a window of k equal bases or an N, left: %s" % (k, 2 * len(r1), windows, left))
        assert 0 < windows < left["pair"] < 2 * len(r1) - 50, (windows, left)
        assert windows < left["lean_first_pass"] < 2 * len(r1) - 50, (windows, left)
    _run_single(rd["idx"], oracle_mod, mh.odd_single(r1, r2), variant, "run reads single-end, k=%d %s" % (k, variant))


@pytest.mark.parametrize("read_len,ns,n", [(150, 3, 500), (250, 4, 300)])
@pytest.mark.parametrize("k", [15, 21])
def test_long_reads_take_the_wide_editions(root, oracle_mod, k, read_len, ns, n):
    """2 x 150 and 2 x 250 characters on the small transcriptome: the three- and four-slot instantiations of the general kernel and, inside
    the emulation, the wide lean kernel (one read per wavefront) held against it word for word"""
    idx = kc.small_index(root, k, "dense")
    q1, o1, q2, o2 = kc.long_reads(root, read_len, n, seed=read_len + k)
    res, er = _run(idx, oracle_mod, q1, o1, q2, o2, "default", "%d bp, k=%d" % (read_len, k), ns=ns)
    assert res.counters["totHits"] > n
    _run(idx, oracle_mod, q1, o1, q2, o2, "selAln", "%d bp -s, k=%d" % (read_len, k), ns=ns)
    ix, orc, em = mh.emu_of(idx)
    rs = orc.map_single(q2[: o2[-2]], o2[:-1], nthreads=4)
    es = em.map(q2[: o2[-2]], o2[:-1], ns=ns)
    assert es.status == 0
    mh.check(rs, es, "%d bp single-end, k=%d" % (read_len, k))


@pytest.mark.parametrize("k", kc.KS)
def test_error_free_pairs_hold_their_true_position(root, oracle_mod, k):
    """2 000 error-free pairs: every pair's own transcript and position is among the emulation's hits (a plain search of the transcript
    for the mates' characters; no oracle, no suffix array)"""
    idx = kc.small_index(root, k, "dense")
    q1, o1, q2, o2, truth = kc.truth_pairs(root)
    ix, orc, em = mh.emu_of(idx)
    er = em.map(q1, o1, q2, o2)
    assert er.status == 0
    kc.truth_check(er.hit_offsets, er.hits, truth, kc.txp_seqs_of(idx))
