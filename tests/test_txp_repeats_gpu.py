"""Transcripts that repeat inside themselves (repeat_cases.py) on the HIP path (libqmap_mi355.so through its C ABI), against the oracle:
bit-exact hits, offsets, counters and -- where the general kernel keeps them -- SA-interval lists.  The lane emulation of the same
source runs the same data in test_txp_repeats.py; what only this module sees is the host's choice of the slot class for a batch that
holds one longer read (the 100-character reads then run at ns = 3, 4 or 8, or next to the long-read pass), the real LDS staging of a
first interval's records, the packed table builders on periodic text, and the consumers of the hits on the device (equivalence classes,
fragment lengths).

Every index is built once per module, every oracle result once (shared, never changed); each test prints what it ran and how long the
device calls took."""
import numpy as np
import pytest

import eqc_cases as eqc
import mapping_harness as mh
import rapmap_amd as ra
import repeat_cases as rc
from util import pack

pytestmark = pytest.mark.gpu

HEADLINE_SETS = ("default", "fuzzy", "noDovetail", "noOrphans", "m3", "maxInterval50", "selAln")


@pytest.fixture(scope="module")
def root(tmp_path_factory, lib_built, oracle_mod):
    return tmp_path_factory.mktemp("txp_repeats_gpu")


def test_general_kernel_k31(root, oracle_mod):
    """every option set at k = 31, 2 x 100, with the interval lists where -s is off"""
    mh.general_kernel(rc, root, oracle_mod, 31, 100, "dense", rc.VARIANTS, timed=True)


@pytest.mark.parametrize("k,L,image,ph_compact", [(21, 100, "dense", False), (15, 100, "dense", False), (31, 100, "ph", False), (31, 100, "ph", True),
                                                  (31, 64, "dense", False), (31, 150, "dense", False), (31, 250, "dense", False)])
def test_general_kernel_other_shapes(root, oracle_mod, k, L, image, ph_compact):
    mh.general_kernel(rc, root, oracle_mod, k, L, image, rc.FEW, ph_compact=ph_compact, timed=True)


@pytest.mark.parametrize("kernel", mh.HEADLINE_KERNELS)
@pytest.mark.parametrize("k", [31, 21, 15])
def test_headline_kernels(root, oracle_mod, k, kernel):
    """the pair kernel and qm_lean_kernel: their per-transcript minimum over the parked suffixes; they leave exactly the reads the lane
    emulation of the same source leaves (repeat_cases.EXPECT_LEFT), and the pair kernel merged some pairs itself"""
    idx = rc.index_for(root, k, "dense")
    with mh.headline(idx, kernel) as (qi, mp):
        for variant in HEADLINE_SETS if k == 31 else ("default",):
            r = mh.ref(rc, root, oracle_mod, k, 100, "dense", variant)
            what, n = r.what, r.n
            tm = mh.Timer("%s kernel, %s" % (kernel, what))
            gr = mp.map_pairs(*r.a, opts=mh.lib_opts(variant, oracle_mod))
            mh.check(r.res, gr, tm.what)
            tm.done(1)
            if not mh.is_sel(variant):
                assert mp.stat(ra.QM_STAT_LEAN_READS) == 2 * n, "the %s kernel did not run" % kernel
            if variant == "default":
                assert mp.stat(ra.QM_STAT_LEAN_DEFERRED) == rc.EXPECT_LEFT[(k, "dense")][kernel], mp.stat(ra.QM_STAT_LEAN_DEFERRED)
                if kernel == "pair":
                    merged = mp.stat(ra.QM_STAT_PAIRS_MERGED)
                    print("pair kernel, %s: merged %d of %d pairs itself" % (what, merged, n))
                    assert merged > 0


def test_lean_kernel_compact_ph(root, oracle_mod):
    """the compact -p image, where the host launches qm_lean_kernel's PH edition"""
    mh.lean_kernel_compact_ph(rc, root, oracle_mod, 31, lean_sets=("default",), expect_left=rc.EXPECT_LEFT[(31, "ph_compact")]["lean"], timed=True)


@pytest.mark.parametrize("L", [150, 250])
def test_wide_lean_kernel(root, oracle_mod, L):
    """reads of 150 and 250 characters: the wide lean kernel (one read per wavefront), paired and single-end; -s with its slow pass"""
    mh.wide_lean_kernel(rc, root, oracle_mod, 31, L, slow_pass=True, timed=True)


@pytest.mark.parametrize("debug", [True, False])
def test_single_end(root, oracle_mod, debug):
    """single-end, an odd count, through the general kernel and the lean kernel: the raw negative positions"""
    mh.single_end(rc, root, oracle_mod, debug, lean_sets=("default",), timed=True)


@pytest.mark.parametrize("debug", [True, False])
@pytest.mark.parametrize("extra", [150, 250, 300, 600])
def test_one_longer_pair_in_the_batch(root, oracle_mod, extra, debug):
    """the 100-character pairs and one pair of 150 (ns = 3), 250 (ns = 4), 300 (ns = 8) or 600 characters (the long-read pass) in one call:
    the host picks the slot class by the longest read, and the staging of a first interval's records then reaches beyond 64 suffixes"""
    idx = rc.index_for(root, 31, "dense")
    with mh.gpu_mapper(idx, debug=debug) as (qi, mp):
        tm = mh.Timer("one pair of %d behind the pairs of 100, debug=%s" % (extra, debug))
        for variant in ("default", "fuzzy", "selAln"):
            ints = debug and not mh.is_sel(variant)
            r = mh.ref(rc, root, oracle_mod, 31, 100, "dense", variant, ints=ints, extra=extra)
            gr = mp.map_pairs(*r.a, opts=mh.lib_opts(variant, oracle_mod))
            mh.check(r.res, gr, "%s, debug=%s" % (r.what, debug), ints=mp.intervals(r.n) if ints else None)
        tm.done(3)


@pytest.mark.parametrize("extra", [0, 150])
def test_device_resident_inputs(root, oracle_mod, extra):
    """qm_map_device: the reads already in device memory, the slot class from the caller's max_read_len"""
    import torch
    r = mh.ref(rc, root, oracle_mod, 31, 100, "dense", "default", extra=extra)
    a, n = r.a, r.n
    pad = np.zeros(8, np.uint8)
    d = [torch.from_numpy(np.concatenate([a[0], pad])).cuda(), torch.from_numpy(a[1]).cuda(), torch.from_numpy(np.concatenate([a[2], pad])).cuda(), torch.from_numpy(a[3]).cuda()]
    torch.cuda.synchronize()
    with mh.gpu_mapper(r.idx, debug=False) as (qi, mp):
        tm = mh.Timer("device-resident, " + r.what)
        gr = mp.map_device(n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), max(100, extra), fetch=True)
        mh.check(r.res, gr, tm.what)
        tm.done(1)


@pytest.mark.parametrize("kernel", mh.HEADLINE_KERNELS)
def test_reads_with_N_inside_an_array(root, oracle_mod, kernel, monkeypatch):
    """a few pairs with an N inside an array: the N-aware second pass of the lean kernel (QM_NPASS_MIN: 2 048, here 1), default and -s"""
    monkeypatch.setenv("QM_NPASS_MIN", "1")
    idx = rc.index_for(root, 31, "dense")
    r1, r2 = rc.n_reads(31, 100)
    a = pack(r1) + pack(r2)
    orc = mh.oracle_of(idx)[1]
    with mh.headline(idx, kernel) as (qi, mp):
        tm = mh.Timer("%d pairs with an N, behind the %s kernel" % (len(r1), kernel))
        for variant in ("default", "selAln"):
            oopts, gopts = mh.opts_for(variant, oracle_mod, ra.default_opts)
            res = orc.map_pairs(*a, opts=oopts, nthreads=8)
            gr = mp.map_pairs(*a, opts=gopts)
            mh.check(res, gr, "%s, %s" % (tm.what, variant))
            taken = mp.stat(ra.QM_STAT_N_PASS_READS)
            print("%s, %s: the N-aware pass mapped %d reads, %d hits" % (tm.what, variant, taken, len(res.hits)))
            assert taken > 0 and len(res.hits) > len(r1) // 2
        tm.done(2)


def test_packed_reads_and_stage_view(root, oracle_mod):
    """the reads sent 2-bit packed (map_pairs_packed) give the fused result; the stage entry points (map_pairs_stages, with and without
    intervals, reads as characters and packed) give it unit by unit but for the units whose excess orphans only the caller drops"""
    mh.packed_reads_and_stage_view(rc, root, oracle_mod, expect_left=rc.EXPECT_LEFT[(31, "dense")]["pair"], timed=True)


def test_table_builders(root, oracle_mod, monkeypatch):
    """QM_TABLE_CHECK=1 holds every entry of SaExt / SaExt2 / sanext as the packed builders made it against the byte-per-character builders
    and fails the build on a difference -- on periodic text, where the characters behind a k-mer are the same for hundreds of suffixes in
    a row: one -s call (sanext), one with 150-character reads (SaExt2), and one with 100-character reads on a fresh mapper (SaExt alone)"""
    monkeypatch.setenv("QM_TABLE_CHECK", "1")
    mh.table_builders(rc, root, oracle_mod, 31, timed=True)


@pytest.mark.parametrize("kernel", ["general", "pair"])
def test_leftmost_positions(root, oracle_mod, kernel):
    """repeat_cases.truth_check on the DEVICE's hits: no oracle, no suffix array"""
    idx = rc.index_for(root, 31, "dense")
    rd, tx = rc.reads_for(31, 100), rc.txome(31)
    with mh.gpu_mapper(idx, debug=kernel == "general") as (qi, mp):
        tm = mh.Timer("truth_check, %s kernel" % kernel)
        gr = mp.map_pairs(rd["q1"], rd["o1"], rd["q2"], rd["o2"])
        assert mp.stat(ra.QM_STAT_LEAN_READS) == (-1 if kernel == "general" else 2 * rd["n"])
        got = rc.truth_check(gr.hit_offsets, gr.hits, rd, tx, 31)
        print("truth_check, %s kernel, paired: %d eligible mates, %d checked, %d at a negative position, left out %r" % ((kernel,) + got))
        gs = mp.map_reads(*pack(mh.odd_single(rd["r1"], rd["r2"])))
        got = rc.truth_check(gs.hit_offsets, gs.hits, rd, tx, 31, single=True)
        print("truth_check, %s kernel, single-end: %d eligible mates, %d checked, %d at a negative position, left out %r" % ((kernel,) + got))
        tm.done(2)


@pytest.mark.parametrize("variant", ["default", "fuzzy"])
def test_equivalence_classes(root, oracle_mod, variant):
    """the device's fold of the mapped batch against eqc_cases.expected of the oracle's hits; every label is ascending and distinct.  (On
    this data no unit of the oracle's lists one transcript twice, not under fuzzy either -- a transcript hit in both orientations is one
    record by the time the pair is merged -- so the count printed below is 0: the fold's own removal of repeats is test_eq_classes_gpu's.)"""
    r = mh.ref(rc, root, oracle_mod, 31, 100, "dense", variant)
    idx, a, n, res, what = r.idx, r.a, r.n, r.res, r.what
    want = eqc.expected_from_hits(res.hit_offsets, res.hits)
    tid = res.hits["tid"]
    twice = sum(len(set(tid[res.hit_offsets[u]:res.hit_offsets[u + 1]].tolist())) < res.hit_offsets[u + 1] - res.hit_offsets[u] for u in range(n))
    with mh.gpu_mapper(idx, debug=False) as (qi, mp):
        tm = mh.Timer("equivalence classes, " + what)
        mp.map_pairs(*a, opts=mh.lib_opts(variant, oracle_mod))
        t = ra.EqClasses(mp)
        try:
            t.add(mp)
            off, tids, cnt = t.fetch()
            eqc.assert_table((off, tids, cnt), want, what)
            for c in range(len(off) - 1):
                assert (np.diff(tids[off[c]:off[c + 1]].astype(np.int64)) > 0).all(), "label %d is not ascending and distinct" % c
        finally:
            t.close()
        tm.done(1)
    print("equivalence classes, %s: %d classes, %d units list a transcript more than once" % (what, len(want), twice))


def test_fragment_lengths(root, oracle_mod):
    """the device's histogram over the default mapping equals fld_cases' restatement over the oracle's hits: mates that choose different
    copies of a unit give fragment lengths nothing else produces"""
    mh.fragment_lengths(rc, root, oracle_mod, timed=True)
