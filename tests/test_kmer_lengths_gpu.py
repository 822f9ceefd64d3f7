"""The HIP path (libqmap_mi355.so through its C ABI) at k-mer lengths other than 31, against the oracle: bit-exact hits, offsets,
counters and -- where the general kernel keeps them -- SA-interval lists.  Everything else that maps a read in this suite does so at
k = 31; here the general kernel, the pair and lean kernels, the N-aware pass, the wide lean kernel, the table builders, the packed
upload, the stage view and the command line run at k = 15, 17, 21 and 29.  Data and checks are in kmer_cases.py; the same cases run
under the lane emulation in test_kmer_lengths.py.

The reference is the oracle, which reads k from the index header: the reference's own binary cannot be built here, so there is no
golden SAM at another k.  test_error_free_pairs_* is the one check that does not go through the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kmer_cases as kc
import mapping_harness as mh
import rapmap_amd as ra
from conftest import GOLD, ROOT, load_oracle
from util import pack

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def root(tmp_path_factory, lib_built, oracle_mod):
    return tmp_path_factory.mktemp("kmer_lengths_gpu")


def _opts(oracle_mod, variant):
    return mh.opts_for(variant, oracle_mod, ra.default_opts)


@pytest.mark.parametrize("image", ["dense", "ph"])
@pytest.mark.parametrize("k", kc.KS)
def test_general_kernel(root, oracle_mod, k, image):
    """the golden reads through the general stage-A kernel (intervals kept): hits, counters and the interval lists"""
    idx = kc.index_for(root, k, image)
    orc = mh.oracle_of(idx)[1]
    q1, o1, q2, o2 = kc.golden_reads()[4]
    with mh.gpu_mapper(idx, debug=True) as (qi, mp):
        assert qi.perfect_hash == (image == "ph")
        for variant in sorted(kc.FEW):
            oopts, gopts = _opts(oracle_mod, variant)
            ints = variant != "selAln"
            res = orc.map_pairs(q1, o1, q2, o2, opts=oopts, nthreads=8, want_ints=ints)
            gr = mp.map_pairs(q1, o1, q2, o2, opts=gopts)
            if ints:                                     # (with -s the lean kernel's collector edition writes the interval records itself)
                assert mp.stat(ra.QM_STAT_LEAN_READS) == -1, "expected the general kernel"
            mh.check(res, gr, "general kernel, k=%d %s %s" % (k, image, variant), ints=mp.intervals(len(o1) - 1) if ints else None)
            assert res.counters["peHits"] > 1000


@pytest.mark.parametrize("kernel", mh.HEADLINE_KERNELS)
@pytest.mark.parametrize("k", kc.KS)
def test_headline_kernels(root, oracle_mod, k, kernel):
    """the golden reads through the pair kernel and qm_lean_kernel: what they take is right, they leave what they are not built for, and
    they leave exactly the reads the lane emulation of the same source leaves (kmer_cases.EXPECT_LEFT) -- dense table and compact -p image"""
    q1, o1, q2, o2 = kc.golden_reads()[4]
    n = len(o1) - 1
    idx = kc.index_for(root, k, "dense")
    orc = mh.oracle_of(idx)[1]
    with mh.headline(idx, kernel) as (qi, mp):
        for variant in ("default", "noStrictCheck", "z0.9"):
            oopts, gopts = _opts(oracle_mod, variant)
            res = orc.map_pairs(q1, o1, q2, o2, opts=oopts, nthreads=8)
            gr = mp.map_pairs(q1, o1, q2, o2, opts=gopts)
            mh.check(res, gr, "%s kernel, k=%d %s" % (kernel, k, variant))
            deferred = mh.check_headline(mp, kernel, n)
            if variant == "default":
                assert deferred == kc.EXPECT_LEFT[(k, "dense")][kernel], deferred
    # the compact -p image: the host never picks the pair kernel there (plan_stage_a: a lane per position would serialise the two BooPHF
    # walks), so either mapper runs qm_lean_kernel's PH edition
    idx = kc.index_for(root, k, "ph")
    orc = mh.oracle_of(idx)[1]
    with mh.headline(idx, kernel, ph_compact=True) as (qi, mp):
        assert qi.perfect_hash
        res = orc.map_pairs(q1, o1, q2, o2, nthreads=8)
        gr = mp.map_pairs(q1, o1, q2, o2)
        mh.check(res, gr, "%s kernel, compact -p, k=%d" % (kernel, k))
        assert mh.check_headline(mp, "lean", n) == kc.EXPECT_LEFT[(k, "ph")]["lean"]


@pytest.mark.parametrize("kernel", mh.HEADLINE_KERNELS + ["general"])
@pytest.mark.parametrize("k", kc.KS)
def test_edge_and_run_reads(root, oracle_mod, k, kernel):
    """kmer_cases.edge_reads and run_reads through both headline kernels, and through the general kernel with --noSensitive: paired, and
    single-end with an odd count"""
    gidx = kc.index_for(root, k, "dense")
    rd = kc.run_reads(root, k)
    for name, idx, (r1, r2) in (("edge", gidx, kc.edge_reads(gidx, k)), ("run", rd["idx"], (rd["reads1"], rd["reads2"]))):
        orc = mh.oracle_of(idx)[1]
        q1, o1 = pack(r1); q2, o2 = pack(r2)
        qs, os_ = pack(mh.odd_single(r1, r2))
        assert (len(os_) - 1) % 2 == 1
        what = "%s reads, %s kernel, k=%d" % (name, kernel, k)
        if kernel == "general":
            oopts, gopts = _opts(oracle_mod, "noSensitive")
            with mh.gpu_mapper(idx, debug=True) as (qi, mp):
                res = orc.map_pairs(q1, o1, q2, o2, opts=oopts, nthreads=4, want_ints=True)
                gr = mp.map_pairs(q1, o1, q2, o2, opts=gopts)
                assert mp.stat(ra.QM_STAT_LEAN_READS) == -1
                mh.check(res, gr, what, ints=mp.intervals(len(o1) - 1))
                rs = orc.map_single(qs, os_, opts=oopts, nthreads=4)
                gs = mp.map_reads(qs, os_, opts=gopts)
                mh.check(rs, gs, what + ", single-end")
        else:
            with mh.headline(idx, kernel) as (qi, mp):
                res = orc.map_pairs(q1, o1, q2, o2, nthreads=4)
                gr = mp.map_pairs(q1, o1, q2, o2)
                mh.check(res, gr, what)
                mh.check_headline(mp, kernel, len(r1), some_merged=False)
                rs = orc.map_single(qs, os_, nthreads=4)
                gs = mp.map_reads(qs, os_)
                mh.check(rs, gs, what + ", single-end")
                assert mp.stat(ra.QM_STAT_LEAN_READS) == len(os_) - 1 and 0 < mp.stat(ra.QM_STAT_LEAN_DEFERRED) < len(os_) - 1


@pytest.mark.parametrize("kernel", mh.HEADLINE_KERNELS)
@pytest.mark.parametrize("k", [15, 21])
def test_n_aware_pass(root, oracle_mod, k, kernel, monkeypatch):
    """the golden reads and edge_reads' N cases (an N at k, at k - 1, at L - k - 1) with the N-aware edition of qm_lean_kernel going over
    what the first pass left (QM_NPASS_MIN=1: also on a small batch): kmask = (1 << k) - 1 and (nb >> k) & 1 at k below 31"""
    monkeypatch.setenv("QM_NPASS_MIN", "1")
    idx = kc.index_for(root, k, "dense")
    orc = mh.oracle_of(idx)[1]
    g = kc.golden_reads()
    n1, n2 = kc.n_case_reads(idx, k)
    assert len(n1) > 100
    q1, o1 = pack(list(g[1]) + n1); q2, o2 = pack(list(g[3]) + n2)
    with mh.headline(idx, kernel) as (qi, mp):
        for variant in ("default", "selAln"):
            oopts, gopts = _opts(oracle_mod, variant)
            res = orc.map_pairs(q1, o1, q2, o2, opts=oopts, nthreads=8)
            gr = mp.map_pairs(q1, o1, q2, o2, opts=gopts)
            mh.check(res, gr, "N-aware pass behind the %s kernel, k=%d %s" % (kernel, k, variant))
            taken = mp.stat(ra.QM_STAT_N_PASS_READS)
            assert taken > 100, taken
        qs, os_ = pack(mh.odd_single(n1, n2))
        rs = orc.map_single(qs, os_, nthreads=4)
        gs = mp.map_reads(qs, os_)
        mh.check(rs, gs, "N-aware pass, single-end, k=%d" % k)
        assert mp.stat(ra.QM_STAT_N_PASS_READS) > 0


@pytest.mark.parametrize("k", [15, 21, 29])
def test_table_builders(root, oracle_mod, k, monkeypatch):
    """SaExt / SaExt2 / sanext are built from a 2-bit image of the text at SA[i] + k; QM_TABLE_CHECK=1 holds every entry against the
    byte-per-character builders on the device and fails the build on a difference.  One -s call (sanext), one call with 150-character
    reads (the wide table is there and the wide lean kernel ran)"""
    monkeypatch.setenv("QM_TABLE_CHECK", "1")
    idx = kc.small_index(root, k, "dense")
    orc = mh.oracle_of(idx)[1]
    with mh.gpu_mapper(idx, debug=False, wide_reads=True) as (qi, mp):
        q1, o1, q2, o2 = kc.long_reads(root, 100, 1500, seed=7)
        gr = mp.map_pairs(q1, o1, q2, o2, opts=ra.default_opts(sel_aln=1))
        res = orc.map_pairs(q1, o1, q2, o2, opts=oracle_mod.default_opts(selAln=1), nthreads=8)
        mh.check(res, gr, "-s with checked tables, k=%d" % k)
        assert res.counters["totHits"] > 1000
        w1, wo1, w2, wo2 = kc.long_reads(root, 150, 500, seed=77)
        gw = mp.map_pairs(w1, wo1, w2, wo2)
        rw = orc.map_pairs(w1, wo1, w2, wo2, nthreads=8)
        mh.check(rw, gw, "150 bp with checked tables, k=%d" % k)
        assert mp.stat(ra.QM_STAT_LEAN_READS) == 2 * 500, "the wide lean kernel did not run: no SaExt2"


@pytest.mark.parametrize("max_len", [150, 256])
@pytest.mark.parametrize("k", [17, 29])
def test_wide_lean_kernel(root, oracle_mod, k, max_len):
    """the lean kernel's wide edition (one read of up to 256 characters per wavefront) on ragged, dirty reads whose ordinary lengths start
    at max(k, max_len // 3): dense table and compact -p image, default and -s, paired and single-end with an odd count"""
    n = 1501
    text, offsets = kc.index_text(kc.small_index(root, k, "dense"))
    r1, r2 = kc.fuzz_reads(text, offsets, n, 4200 + max_len + k, max_len, k)
    q1, o1 = pack(r1); q2, o2 = pack(r2)
    assert 128 < int(np.diff(o1).max()) <= max_len
    for image, compact in (("dense", False), ("ph", True)):
        idx = kc.small_index(root, k, image)
        orc = mh.oracle_of(idx)[1]
        with mh.gpu_mapper(idx, debug=False, ph_compact=compact) as (qi, mp):
            for variant in ("default", "selAln"):
                oopts, gopts = _opts(oracle_mod, variant)
                what = "wide lean, k=%d, <= %d, %s %s" % (k, max_len, image, variant)
                res = orc.map_pairs(q1, o1, q2, o2, opts=oopts, nthreads=8)
                gr = mp.map_pairs(q1, o1, q2, o2, opts=gopts)
                mh.check(res, gr, what)
                if variant == "default":
                    assert mp.stat(ra.QM_STAT_LEAN_READS) == 2 * n, "the lean kernel was not the one launched"
                    assert 0 < mp.stat(ra.QM_STAT_LEAN_DEFERRED) < n, "expected most reads taken, some left to the general kernel"
                rs = orc.map_single(q2, o2, opts=oopts, nthreads=8)
                gs = mp.map_reads(q2, o2, opts=gopts)
                mh.check(rs, gs, what + ", single-end")


def test_packed_upload_k21(root, oracle_mod):
    """qm_map_pairs_packed (reads sent 2-bit packed, unpacked on the device) gives what qm_map_pairs gives, at k = 21"""
    idx = kc.index_for(root, 21, "dense")
    orc = mh.oracle_of(idx)[1]
    q1, o1, q2, o2 = kc.golden_reads()[4]
    with mh.gpu_mapper(idx, debug=False) as (qi, mp):
        for variant in ("default", "selAln"):
            oopts, gopts = _opts(oracle_mod, variant)
            res = orc.map_pairs(q1, o1, q2, o2, opts=oopts, nthreads=8)
            plain = mp.map_pairs(q1, o1, q2, o2, opts=gopts)
            hits, offs, ctr = plain.hits.copy(), plain.hit_offsets.copy(), dict(plain.counters)
            gr = mp.map_pairs_packed(q1, o1, q2, o2, opts=gopts)
            assert np.array_equal(offs, gr.hit_offsets) and hits.tobytes() == gr.hits.tobytes() and ctr == gr.counters
            mh.check(res, gr, "packed pairs, k=21 %s" % variant)
        rs = orc.map_single(q2, o2, nthreads=8)
        mh.check(rs, mp.map_reads_packed(q2, o2), "packed single-end, k=21")


def test_stage_view_k21(root, oracle_mod):
    """k = 21.  The driver's fused path (map_pairs) gives the oracle's hits, offsets and counters.  The stage view -- the interval-keeping
    pass on the general kernel, and map_pairs_stages(no_intervals=True) on the pair / lean kernels, reads as characters and 2-bit packed --
    gives the same records and counters as that fused result in every unit but those whose more than maxNumHits orphans only the
    caller's bookkeeping drops (kmer_cases.check_stage_view).  The interval-keeping pass's intervals are the oracle's, and the pass
    without intervals equals it in every other stage output: foundHit, lists, hits, tooMany flags."""
    idx = kc.index_for(root, 21, "dense")
    orc = mh.oracle_of(idx)[1]
    q1, o1, q2, o2 = kc.golden_reads()[4]
    n = len(o1) - 1
    res = orc.map_pairs(q1, o1, q2, o2, nthreads=8, want_ints=True)
    with mh.gpu_mapper(idx, debug=False) as (qi, mp):
        fused = mp.map_pairs(q1, o1, q2, o2)
        mh.check(res, fused, "fused driver path, k=21")
        fused_hits, fused_off, fused_ctr = fused.hits.copy(), fused.hit_offsets.copy(), dict(fused.counters)
        full = mp.map_pairs_stages(q1, o1, q2, o2)
        mh.check_stage_view(res, full, "stage view with intervals, k=21")
        vf = {key: (np.array(v, copy=True) if hasattr(v, "shape") else v) for key, v in mp.fetch_stages(pinned=False).items()}
        assert mp.stat(ra.QM_STAT_LEAN_READS) == -1
        fo, fi = mp.intervals(n)
        mh.check_intervals(res, fo, fi, "stage view with intervals, k=21")
        full_hits, full_off, full_ctr = full.hits.copy(), full.hit_offsets.copy(), dict(full.counters)
        for packed in (False, True):
            light = mp.map_pairs_stages(q1, o1, q2, o2, no_intervals=True, packed=packed)
            assert mp.stat(ra.QM_STAT_LEAN_READS) == 2 * n and mp.stat(ra.QM_STAT_LEAN_DEFERRED) == kc.EXPECT_LEFT[(21, "dense")]["pair"], "the lean / pair kernel did not run"
            v = mp.fetch_stages(pinned=packed)
            assert np.array_equal(light.hit_offsets, full_off) and light.hits.tobytes() == full_hits.tobytes() and light.counters == full_ctr
            dropped = mh.check_stage_view(res, light, "stage view without intervals, packed=%s, k=21" % packed)
            if dropped == 0:                             # nothing for the caller's bookkeeping to do: the fused result itself
                assert np.array_equal(light.hit_offsets, fused_off) and light.hits.tobytes() == fused_hits.tobytes() and light.counters == fused_ctr
            assert int(v["iv_off"][-1]) == 0 and v["iv"].size == 0
            assert np.array_equal(v["found"], vf["found"])
            assert np.array_equal(v["list_off"], vf["list_off"]) and np.array_equal(v["words"], vf["words"])
            assert np.array_equal(v["hit_off"], vf["hit_off"]) and v["hits"].tobytes() == vf["hits"].tobytes()
            assert np.array_equal(v["too_many"], vf["too_many"])
            mp._arena_cap = 0


@pytest.mark.parametrize("k", kc.KS)
def test_error_free_pairs_hold_their_true_position(root, oracle_mod, k):
    """2 000 error-free pairs: every pair's own transcript and position is among the device's hits (a plain search of the transcript for
    the mates' characters; no oracle, no suffix array)"""
    idx = kc.small_index(root, k, "dense")
    q1, o1, q2, o2, truth = kc.truth_pairs(root)
    with mh.gpu_mapper(idx, debug=False) as (qi, mp):
        gr = mp.map_pairs(q1, o1, q2, o2)
        assert mp.stat(ra.QM_STAT_LEAN_READS) == 2 * len(truth)
        kc.truth_check(gr.hit_offsets, gr.hits, truth, kc.txp_seqs_of(idx))


def test_cli_k21(root, oracle_mod, tmp_path):
    """`quasiindex -k 21`, then `quasimap` on the golden FASTQ files: the SAM is samfmt over the oracle's hits on that index"""
    import samfmt as sam
    idx = str(tmp_path / "idx21")
    run = lambda args: subprocess.run([sys.executable, "-m", "rapmap_amd"] + args, cwd=ROOT, capture_output=True, text=True)
    r = run(["quasiindex", "-t", kc.golden_fasta(root), "-i", idx, "-k", "21"])
    assert r.returncode == 0, r.stderr
    out = tmp_path / "out.sam"
    gd = os.path.join(GOLD, "synth_small")
    r = run(["quasimap", "-i", idx, "-1", os.path.join(gd, "reads_1.fastq.gz"), "-2", os.path.join(gd, "reads_2.fastq.gz"), "-o", str(out), "-t", "2", "-q"])
    assert r.returncode == 0, r.stderr
    ix, orc = load_oracle(idx)
    assert ix.k == 21
    n1, s1, n2, s2, (q1, o1, q2, o2) = kc.golden_reads()
    res = orc.map_pairs(q1, o1, q2, o2, nthreads=8)
    want = "".join(sam.format_pair(n1[i], s1[i], n2[i], s2[i], res.hits[res.hit_offsets[i]:res.hit_offsets[i + 1]], ix.names, ix.txpLens)
                   for i in range(len(o1) - 1))
    lines = open(out).read().splitlines(True)
    assert "".join(l for l in lines if not l.startswith("@")) == want
    header = "".join(l for l in lines if l.startswith("@") and not l.startswith("@PG"))
    assert header == "".join(l for l in sam.sam_header(ix.names, ix.txpLens).splitlines(True) if not l.startswith("@PG"))
