"""Transcripts that repeat inside themselves (repeat_cases.py) on the HIP path (libqmap_mi355.so through its C ABI), against the oracle:
bit-exact hits, offsets, counters and -- where the general kernel keeps them -- SA-interval lists.  The lane emulation of the same
source runs the same data in test_txp_repeats.py; what only this module sees is the host's choice of the slot class for a batch that
holds one longer read (the 100-character reads then run at ns = 3, 4 or 8, or next to the long-read pass), the real LDS staging of a
first interval's records, the packed table builders on periodic text, and the consumers of the hits on the device (equivalence classes,
fragment lengths).

Every index is built once per module, every oracle result once (shared, never changed); each test prints what it ran and how long the
device calls took."""
import contextlib
import time

import numpy as np
import pytest

import eqc_cases as eqc
import fld_cases as fc
import kmer_cases as kc
import repeat_cases as rc
from conftest import load_oracle
from test_gpu_parity import HEADLINE_KERNELS
from test_txp_repeats import EXPECT_LEFT
from util import pack

pytestmark = pytest.mark.gpu

QM_STAT_SLOW, QM_STAT_LEAN_READS, QM_STAT_LEAN_DEFERRED, QM_STAT_PAIRS_MERGED, QM_STAT_NPASS = 2, 3, 4, 10, 15      # include/qmap_mi355.h
HEADLINE_SETS = ("default", "fuzzy", "noDovetail", "noOrphans", "m3", "maxInterval50", "selAln")

_oracles, _refs = {}, {}


def _oracle(idx):
    if idx not in _oracles:
        _oracles[idx] = load_oracle(idx)
    return _oracles[idx]


@pytest.fixture(scope="module")
def root(tmp_path_factory, lib_built, oracle_mod):
    return tmp_path_factory.mktemp("txp_repeats_gpu")


@contextlib.contextmanager
def _gpu(idx, debug=True, ph_compact=False, pair_kernel=True, wide_reads=False):
    """as test_gpu_parity._gpu: debug=True keeps the SA-interval records and so runs the GENERAL stage-A kernel; closed on the way out"""
    import rapmap_amd as ra
    qi = ra.QuasiIndex(idx)
    try:
        mp = ra.QuasiMapper(qi, 0, debug=debug, ph_compact=ph_compact, pair_kernel=pair_kernel, wide_reads=wide_reads)
        try:
            yield qi, mp
        finally:
            mp.close()
    finally:
        qi.close()


def _gopts(variant, oracle_mod):
    import rapmap_amd as ra
    return rc.opts_for(variant, oracle_mod, ra.default_opts)[1]


def _sel(variant):
    return variant.startswith("selAln") or variant.startswith("mimic")


def _ref(root, oracle_mod, k, L, image, variant, single=False, ints=False, extra=0):
    """the oracle's result of one configuration, computed once and shared -> (idx, packed reads (q1, o1, q2, o2) or (q, o), units, result, what).
    extra: the pairs of reads_for(k, L) with one pair of `extra` characters appended (repeat_cases.mixed)"""
    import rapmap_amd as ra
    key = (k, L, image, variant, single, ints, extra)
    idx = rc.index_for(root, k, image)
    rd = rc.reads_for(k, L)
    if single:
        a = pack(rc.odd_single(rd["r1"], rd["r2"]))
    elif extra:
        a = rc.mixed(k, L, extra)
    else:
        a = (rd["q1"], rd["o1"], rd["q2"], rd["o2"])
    if key not in _refs:
        oopts, _ = rc.opts_for(variant, oracle_mod, ra.default_opts)
        orc = _oracle(idx)[1]
        _refs[key] = orc.map_single(*a, opts=oopts, nthreads=8) if single else orc.map_pairs(*a, opts=oopts, nthreads=8, want_ints=ints)
    what = "k=%d L=%d%s %s %s%s" % (k, L, " + one pair of %d" % extra if extra else "", image, variant, ", single-end" if single else "")
    return idx, a, len(a[1]) - 1, _refs[key], what


class _Timer:
    def __init__(self, what):
        self.what, self.t0 = what, time.perf_counter()

    def done(self, calls):
        print("%s: %d device calls, %.2f s" % (self.what, calls, time.perf_counter() - self.t0))


def _general(root, oracle_mod, k, L, image, variants, ph_compact=False):
    idx = rc.index_for(root, k, image)
    with _gpu(idx, debug=True, ph_compact=ph_compact) as (qi, mp):
        assert qi.perfect_hash == (image == "ph")
        for variant in variants:
            ints = not _sel(variant)
            idx, a, n, res, what = _ref(root, oracle_mod, k, L, image, variant, ints=ints)
            tm = _Timer("general kernel, " + what + (", compact" if ph_compact else ""))
            gr = mp.map_pairs(*a, opts=_gopts(variant, oracle_mod))
            if ints:                                     # (with -s the lean kernel's collector edition writes the interval records itself)
                assert mp.stat(QM_STAT_LEAN_READS) == -1, "expected the general kernel"
            rc.check(res, gr, tm.what, ints=mp.intervals(n) if ints else None)
            tm.done(1)


def test_general_kernel_k31(root, oracle_mod):
    """every option set at k = 31, 2 x 100, with the interval lists where -s is off"""
    _general(root, oracle_mod, 31, 100, "dense", rc.VARIANTS)


@pytest.mark.parametrize("k,L,image,ph_compact", [(21, 100, "dense", False), (15, 100, "dense", False), (31, 100, "ph", False), (31, 100, "ph", True),
                                                  (31, 64, "dense", False), (31, 150, "dense", False), (31, 250, "dense", False)])
def test_general_kernel_other_shapes(root, oracle_mod, k, L, image, ph_compact):
    _general(root, oracle_mod, k, L, image, rc.FEW, ph_compact=ph_compact)


@pytest.mark.parametrize("kernel", HEADLINE_KERNELS)
@pytest.mark.parametrize("k", [31, 21, 15])
def test_headline_kernels(root, oracle_mod, k, kernel):
    """the pair kernel and qm_lean_kernel: their per-transcript minimum over the parked suffixes; they leave exactly the reads the lane
    emulation of the same source leaves (test_txp_repeats.EXPECT_LEFT), and the pair kernel merged some pairs itself"""
    idx = rc.index_for(root, k, "dense")
    with _gpu(idx, debug=False, pair_kernel=kernel == "pair") as (qi, mp):
        for variant in HEADLINE_SETS if k == 31 else ("default",):
            idx, a, n, res, what = _ref(root, oracle_mod, k, 100, "dense", variant)
            tm = _Timer("%s kernel, %s" % (kernel, what))
            gr = mp.map_pairs(*a, opts=_gopts(variant, oracle_mod))
            rc.check(res, gr, tm.what)
            tm.done(1)
            if not _sel(variant):
                assert mp.stat(QM_STAT_LEAN_READS) == 2 * n, "the %s kernel did not run" % kernel
            if variant == "default":
                assert mp.stat(QM_STAT_LEAN_DEFERRED) == EXPECT_LEFT[(k, "dense")][kernel], mp.stat(QM_STAT_LEAN_DEFERRED)
                if kernel == "pair":
                    merged = mp.stat(QM_STAT_PAIRS_MERGED)
                    print("pair kernel, %s: merged %d of %d pairs itself" % (what, merged, n))
                    assert merged > 0


def test_lean_kernel_compact_ph(root, oracle_mod):
    """the compact -p image, where the host launches qm_lean_kernel's PH edition"""
    idx = rc.index_for(root, 31, "ph")
    with _gpu(idx, debug=False, ph_compact=True) as (qi, mp):
        assert qi.perfect_hash
        for variant in ("default", "selAln"):
            idx, a, n, res, what = _ref(root, oracle_mod, 31, 100, "ph", variant)
            tm = _Timer("lean kernel, compact -p, " + what)
            gr = mp.map_pairs(*a, opts=_gopts(variant, oracle_mod))
            rc.check(res, gr, tm.what)
            tm.done(1)
            if variant == "default":
                assert mp.stat(QM_STAT_LEAN_READS) == 2 * n, "the lean kernel did not run"
                assert mp.stat(QM_STAT_LEAN_DEFERRED) == EXPECT_LEFT[(31, "ph_compact")]["lean"], mp.stat(QM_STAT_LEAN_DEFERRED)


@pytest.mark.parametrize("L", [150, 250])
def test_wide_lean_kernel(root, oracle_mod, L):
    """reads of 150 and 250 characters: the wide lean kernel (one read per wavefront), paired and single-end; -s with its slow pass"""
    idx = rc.index_for(root, 31, "dense")
    with _gpu(idx, debug=False) as (qi, mp):
        tm = _Timer("wide lean kernel, L=%d" % L)
        for variant in ("default", "selAln"):
            idx, a, n, res, what = _ref(root, oracle_mod, 31, L, "dense", variant)
            gr = mp.map_pairs(*a, opts=_gopts(variant, oracle_mod))
            rc.check(res, gr, "wide lean kernel, " + what)
            if variant == "default":
                assert mp.stat(QM_STAT_LEAN_READS) == 2 * n, "the wide lean kernel did not run: no SaExt2"
            else:
                print("wide lean kernel, %s: %d reads on the slow path of -s" % (what, mp.stat(QM_STAT_SLOW)))
                assert mp.stat(QM_STAT_SLOW) > 0
            idx, a, n, rs, what = _ref(root, oracle_mod, 31, L, "dense", variant, single=True)
            gs = mp.map_reads(*a, opts=_gopts(variant, oracle_mod))
            rc.check(rs, gs, "wide lean kernel, " + what)
            if variant == "default":
                assert mp.stat(QM_STAT_LEAN_READS) == n
        tm.done(4)


@pytest.mark.parametrize("debug", [True, False])
def test_single_end(root, oracle_mod, debug):
    """single-end, an odd count, through the general kernel and the lean kernel: the raw negative positions"""
    idx = rc.index_for(root, 31, "dense")
    with _gpu(idx, debug=debug) as (qi, mp):
        tm = _Timer("single-end, debug=%s" % debug)
        for variant in ("default", "selAln"):
            idx, a, n, rs, what = _ref(root, oracle_mod, 31, 100, "dense", variant, single=True)
            gs = mp.map_reads(*a, opts=_gopts(variant, oracle_mod))
            rc.check(rs, gs, "%s, debug=%s" % (what, debug))
            if not debug and variant == "default":
                assert mp.stat(QM_STAT_LEAN_READS) == n
        tm.done(2)


@pytest.mark.parametrize("debug", [True, False])
@pytest.mark.parametrize("extra", [150, 250, 300, 600])
def test_one_longer_pair_in_the_batch(root, oracle_mod, extra, debug):
    """the 100-character pairs and one pair of 150 (ns = 3), 250 (ns = 4), 300 (ns = 8) or 600 characters (the long-read pass) in one call:
    the host picks the slot class by the longest read, and the staging of a first interval's records then reaches beyond 64 suffixes"""
    idx = rc.index_for(root, 31, "dense")
    with _gpu(idx, debug=debug) as (qi, mp):
        tm = _Timer("one pair of %d behind the pairs of 100, debug=%s" % (extra, debug))
        for variant in ("default", "fuzzy", "selAln"):
            ints = debug and not _sel(variant)
            idx, a, n, res, what = _ref(root, oracle_mod, 31, 100, "dense", variant, ints=ints, extra=extra)
            gr = mp.map_pairs(*a, opts=_gopts(variant, oracle_mod))
            rc.check(res, gr, "%s, debug=%s" % (what, debug), ints=mp.intervals(n) if ints else None)
        tm.done(3)


@pytest.mark.parametrize("extra", [0, 150])
def test_device_resident_inputs(root, oracle_mod, extra):
    """qm_map_device: the reads already in device memory, the slot class from the caller's max_read_len"""
    import torch
    idx, a, n, res, what = _ref(root, oracle_mod, 31, 100, "dense", "default", extra=extra)
    pad = np.zeros(8, np.uint8)
    d = [torch.from_numpy(np.concatenate([a[0], pad])).cuda(), torch.from_numpy(a[1]).cuda(), torch.from_numpy(np.concatenate([a[2], pad])).cuda(), torch.from_numpy(a[3]).cuda()]
    torch.cuda.synchronize()
    with _gpu(idx, debug=False) as (qi, mp):
        tm = _Timer("device-resident, " + what)
        gr = mp.map_device(n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), max(100, extra), fetch=True)
        rc.check(res, gr, tm.what)
        tm.done(1)


@pytest.mark.parametrize("kernel", HEADLINE_KERNELS)
def test_reads_with_N_inside_an_array(root, oracle_mod, kernel, monkeypatch):
    """a few pairs with an N inside an array: the N-aware second pass of the lean kernel (QM_NPASS_MIN: 2 048, here 1), default and -s"""
    import rapmap_amd as ra
    monkeypatch.setenv("QM_NPASS_MIN", "1")
    idx = rc.index_for(root, 31, "dense")
    r1, r2 = rc.n_reads(31, 100)
    a = pack(r1) + pack(r2)
    orc = _oracle(idx)[1]
    with _gpu(idx, debug=False, pair_kernel=kernel == "pair") as (qi, mp):
        tm = _Timer("%d pairs with an N, behind the %s kernel" % (len(r1), kernel))
        for variant in ("default", "selAln"):
            oopts, gopts = rc.opts_for(variant, oracle_mod, ra.default_opts)
            res = orc.map_pairs(*a, opts=oopts, nthreads=8)
            gr = mp.map_pairs(*a, opts=gopts)
            rc.check(res, gr, "%s, %s" % (tm.what, variant))
            taken = mp.stat(QM_STAT_NPASS)
            print("%s, %s: the N-aware pass mapped %d reads, %d hits" % (tm.what, variant, taken, len(res.hits)))
            assert taken > 0 and len(res.hits) > len(r1) // 2
        tm.done(2)


def test_packed_reads_and_stage_view(root, oracle_mod):
    """the reads sent 2-bit packed (map_pairs_packed) give the fused result; the stage entry points (map_pairs_stages, with and without
    intervals, reads as characters and packed) give it unit by unit but for the units whose excess orphans only the caller drops"""
    idx, a, n, res, what = _ref(root, oracle_mod, 31, 100, "dense", "default")
    with _gpu(idx, debug=False) as (qi, mp):
        tm = _Timer("packed reads and stage view, " + what)
        fused = mp.map_pairs(*a)
        rc.check(res, fused, "fused, " + what)
        gp = mp.map_pairs_packed(*a)
        rc.check(res, gp, "packed pairs, " + what)
        full = mp.map_pairs_stages(*a)
        kc.check_stage_view(res, full, "stage view with intervals, " + what)
        for packed in (False, True):
            light = mp.map_pairs_stages(*a, no_intervals=True, packed=packed)
            assert mp.stat(QM_STAT_LEAN_READS) == 2 * n, "the lean / pair kernel did not run"
            assert mp.stat(QM_STAT_LEAN_DEFERRED) == EXPECT_LEFT[(31, "dense")]["pair"]
            kc.check_stage_view(res, light, "stage view without intervals, packed=%s, %s" % (packed, what))
        tm.done(5)


def test_table_builders(root, oracle_mod, monkeypatch):
    """QM_TABLE_CHECK=1 holds every entry of SaExt / SaExt2 / sanext as the packed builders made it against the byte-per-character builders
    and fails the build on a difference -- on periodic text, where the characters behind a k-mer are the same for hundreds of suffixes in
    a row: one -s call (sanext), one with 150-character reads (SaExt2), and one with 100-character reads on a fresh mapper (SaExt alone)"""
    monkeypatch.setenv("QM_TABLE_CHECK", "1")
    idx = rc.index_for(root, 31, "dense")
    tm = _Timer("checked tables")
    with _gpu(idx, debug=False, wide_reads=True) as (qi, mp):
        idx, a, n, res, what = _ref(root, oracle_mod, 31, 100, "dense", "selAln")
        rc.check(res, mp.map_pairs(*a, opts=_gopts("selAln", oracle_mod)), "checked tables, " + what)
        idx, a, n, res, what = _ref(root, oracle_mod, 31, 150, "dense", "default")
        rc.check(res, mp.map_pairs(*a), "checked tables, " + what)
        assert mp.stat(QM_STAT_LEAN_READS) == 2 * n, "the wide lean kernel did not run: no SaExt2"
    with _gpu(idx, debug=False) as (qi, mp):
        idx, a, n, res, what = _ref(root, oracle_mod, 31, 100, "dense", "default")
        rc.check(res, mp.map_pairs(*a), "checked tables, fresh mapper, " + what)
        assert mp.stat(QM_STAT_LEAN_READS) == 2 * n
    tm.done(3)


@pytest.mark.parametrize("kernel", ["general", "pair"])
def test_leftmost_positions(root, oracle_mod, kernel):
    """repeat_cases.truth_check on the DEVICE's hits: no oracle, no suffix array"""
    idx = rc.index_for(root, 31, "dense")
    rd, tx = rc.reads_for(31, 100), rc.txome(31)
    with _gpu(idx, debug=kernel == "general") as (qi, mp):
        tm = _Timer("truth_check, %s kernel" % kernel)
        gr = mp.map_pairs(rd["q1"], rd["o1"], rd["q2"], rd["o2"])
        assert mp.stat(QM_STAT_LEAN_READS) == (-1 if kernel == "general" else 2 * rd["n"])
        got = rc.truth_check(gr.hit_offsets, gr.hits, rd, tx, 31)
        print("truth_check, %s kernel, paired: %d eligible mates, %d checked, %d at a negative position, left out %r" % ((kernel,) + got))
        gs = mp.map_reads(*pack(rc.odd_single(rd["r1"], rd["r2"])))
        got = rc.truth_check(gs.hit_offsets, gs.hits, rd, tx, 31, single=True)
        print("truth_check, %s kernel, single-end: %d eligible mates, %d checked, %d at a negative position, left out %r" % ((kernel,) + got))
        tm.done(2)


@pytest.mark.parametrize("variant", ["default", "fuzzy"])
def test_equivalence_classes(root, oracle_mod, variant):
    """the device's fold of the mapped batch against eqc_cases.expected of the oracle's hits; every label is ascending and distinct.  (On
    this data no unit of the oracle's lists one transcript twice, not under fuzzy either -- a transcript hit in both orientations is one
    record by the time the pair is merged -- so the count printed below is 0: the fold's own removal of repeats is test_eq_classes_gpu's.)"""
    import rapmap_amd as ra
    idx, a, n, res, what = _ref(root, oracle_mod, 31, 100, "dense", variant)
    want = eqc.expected_from_hits(res.hit_offsets, res.hits)
    tid = res.hits["tid"]
    twice = sum(len(set(tid[res.hit_offsets[u]:res.hit_offsets[u + 1]].tolist())) < res.hit_offsets[u + 1] - res.hit_offsets[u] for u in range(n))
    with _gpu(idx, debug=False) as (qi, mp):
        tm = _Timer("equivalence classes, " + what)
        mp.map_pairs(*a, opts=_gopts(variant, oracle_mod))
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
    import rapmap_amd as ra
    idx, a, n, res, what = _ref(root, oracle_mod, 31, 100, "dense", "default")
    counts, st = fc.classify(res.hit_offsets, res.hits, 1000)
    with _gpu(idx, debug=False) as (qi, mp):
        tm = _Timer("fragment lengths, " + what)
        mp.map_pairs(*a)
        f = ra.FragLenDist(mp)
        try:
            f.add(mp)
            fc.assert_same(f.counts(), f.stat(), counts, st, what + ": the oracle's hits")
            print("fragment lengths, %s: %r" % (what, st))
            assert st["units"] == n and st["used"] >= 100, st
            assert f.eff_lens(qi.txp_lens).tobytes() == fc.eff_lens(counts, qi.txp_lens).tobytes()
        finally:
            f.close()
        tm.done(1)
