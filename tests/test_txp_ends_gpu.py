"""Reads that hang over a transcript end and transcripts shorter than a read (ends_cases.py) on the HIP path (libqmap_mi355.so through its
C ABI), against the oracle: bit-exact hits, offsets, counters and -- where the general kernel keeps them -- SA-interval lists.  The lane
emulation of the same source runs the same data in test_txp_ends.py; what only this module sees is the host's tables, the packed table
builders on a text this small (a `$` right behind many k-mers, the last k-mer ending the text), the real wave execution and the pair
kernel's merge in LDS.

Every index is built once per module, every oracle result once (shared, never changed); every test that maps asserts
ends_cases.reach()'s minimums on the oracle's own result and prints the counts."""
import contextlib

import numpy as np
import pytest

import ends_cases as ec
import fld_cases as fc
import kmer_cases as kc
from conftest import load_oracle
from util import pack

pytestmark = pytest.mark.gpu

QM_STAT_LEAN_READS, QM_STAT_PAIRS_MERGED = 3, 10      # include/qmap_mi355.h
HEADLINE_SETS = ("default", "fuzzy", "noDovetail", "noOrphans", "selAln")

_oracles, _refs = {}, {}


def _oracle(idx):
    if idx not in _oracles:
        _oracles[idx] = load_oracle(idx)[1]
    return _oracles[idx]


@pytest.fixture(scope="module")
def root(tmp_path_factory, lib_built, oracle_mod):
    return tmp_path_factory.mktemp("txp_ends_gpu")


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


def _ref(root, oracle_mod, k, L, image, variant, single=False, ints=False):
    """the oracle's result of one configuration, computed once and shared, with its reach asserted -> (idx, read set, result, what)"""
    import rapmap_amd as ra
    key = (k, L, image, variant, single, ints)
    idx = ec.index_for(root, k, image)
    rd = ec.reads_for(k, L)
    if key not in _refs:
        oopts, _ = ec.opts_for(variant, oracle_mod, ra.default_opts)
        what = "k=%d L=%d %s %s%s" % (k, L, image, variant, ", single-end" if single else "")
        if single:
            q, o = pack(ec.odd_single(rd["r1"], rd["r2"]))
            assert (len(o) - 1) % 2 == 1
            res, n = _oracle(idx).map_single(q, o, opts=oopts, nthreads=8), len(o) - 1
        else:
            res, n = _oracle(idx).map_pairs(rd["q1"], rd["o1"], rd["q2"], rd["o2"], opts=oopts, nthreads=8, want_ints=ints), rd["n"]
        ec.report("oracle, " + what, n, res, ec.assert_reach(res, rd["lens"], L, variant, what))
        _refs[key] = (res, what)
    return (idx, rd) + _refs[key]


def _gopts(variant, oracle_mod):
    import rapmap_amd as ra
    return ec.opts_for(variant, oracle_mod, ra.default_opts)[1]


def _general(root, oracle_mod, k, L, image, variants, ph_compact=False):
    idx = ec.index_for(root, k, image)
    with _gpu(idx, debug=True, ph_compact=ph_compact) as (qi, mp):
        assert qi.perfect_hash == (image == "ph")
        for variant in variants:
            ints = not (variant.startswith("selAln") or variant.startswith("mimic"))
            idx, rd, res, what = _ref(root, oracle_mod, k, L, image, variant, ints=ints)
            gr = mp.map_pairs(rd["q1"], rd["o1"], rd["q2"], rd["o2"], opts=_gopts(variant, oracle_mod))
            if ints:                                     # (with -s the lean kernel's collector edition writes the interval records itself)
                assert mp.stat(QM_STAT_LEAN_READS) == -1, "expected the general kernel"
            ec.check(res, gr, "general kernel, " + what + (", compact" if ph_compact else ""), ints=mp.intervals(rd["n"]) if ints else None)


def test_general_kernel_k31(root, oracle_mod):
    """every option set at k = 31, 2 x 100, with the interval lists where -s is off"""
    _general(root, oracle_mod, 31, 100, "dense", sorted(ec.OPTION_SETS))


@pytest.mark.parametrize("k,L,image,ph_compact", [(21, 100, "dense", False), (21, 100, "ph", False), (21, 100, "ph", True), (31, 64, "dense", False),
                                                  (31, 150, "dense", False), (15, 250, "dense", False)])
def test_general_kernel_other_shapes(root, oracle_mod, k, L, image, ph_compact):
    _general(root, oracle_mod, k, L, image, ec.FEW, ph_compact=ph_compact)


@pytest.mark.parametrize("kernel", ["pair", "lean"])
@pytest.mark.parametrize("k", [31, 21])
def test_headline_kernels(root, oracle_mod, k, kernel):
    """the pair kernel (its own merge: positions clamped at 0 before the dovetail test, the orphan left of the transcript start under
    --noDovetail) and qm_lean_kernel: both ran, and the pair kernel merged some pairs of this data itself"""
    idx = ec.index_for(root, k, "dense")
    with _gpu(idx, debug=False, pair_kernel=kernel == "pair") as (qi, mp):
        for variant in HEADLINE_SETS:
            idx, rd, res, what = _ref(root, oracle_mod, k, 100, "dense", variant)
            gr = mp.map_pairs(rd["q1"], rd["o1"], rd["q2"], rd["o2"], opts=_gopts(variant, oracle_mod))
            ec.check(res, gr, "%s kernel, %s" % (kernel, what))
            assert mp.stat(QM_STAT_LEAN_READS) == 2 * rd["n"], "the %s kernel did not run" % kernel
            if kernel == "pair" and variant == "default":
                merged = mp.stat(QM_STAT_PAIRS_MERGED)
                print("pair kernel, %s: merged %d of %d pairs itself" % (what, merged, rd["n"]))
                assert merged > 0


@pytest.mark.parametrize("k", [31, 21])
def test_lean_kernel_compact_ph(root, oracle_mod, k):
    """the compact -p image, where the host launches qm_lean_kernel's PH edition"""
    idx = ec.index_for(root, k, "ph")
    with _gpu(idx, debug=False, ph_compact=True) as (qi, mp):
        assert qi.perfect_hash
        for variant in ("default", "selAln"):
            idx, rd, res, what = _ref(root, oracle_mod, k, 100, "ph", variant)
            gr = mp.map_pairs(rd["q1"], rd["o1"], rd["q2"], rd["o2"], opts=_gopts(variant, oracle_mod))
            ec.check(res, gr, "lean kernel, compact -p, " + what)
            assert mp.stat(QM_STAT_LEAN_READS) == 2 * rd["n"], "the lean kernel did not run"


@pytest.mark.parametrize("k,L", [(31, 150), (17, 250)])
def test_wide_lean_kernel(root, oracle_mod, k, L):
    """reads of 150 and 250 characters: the wide lean kernel (one read per wavefront) on SaExt2 entries that stop at a `$` after none or a
    few characters; paired and single-end"""
    idx = ec.index_for(root, k, "dense")
    with _gpu(idx, debug=False) as (qi, mp):
        for variant in ("default", "selAln"):
            idx, rd, res, what = _ref(root, oracle_mod, k, L, "dense", variant)
            gr = mp.map_pairs(rd["q1"], rd["o1"], rd["q2"], rd["o2"], opts=_gopts(variant, oracle_mod))
            ec.check(res, gr, "wide lean kernel, " + what)
            if variant == "default":
                assert mp.stat(QM_STAT_LEAN_READS) == 2 * rd["n"], "the wide lean kernel did not run: no SaExt2"
            idx, rd, rs, what = _ref(root, oracle_mod, k, L, "dense", variant, single=True)
            q, o = pack(ec.odd_single(rd["r1"], rd["r2"]))
            gs = mp.map_reads(q, o, opts=_gopts(variant, oracle_mod))
            ec.check(rs, gs, "wide lean kernel, " + what)
            if variant == "default":
                assert mp.stat(QM_STAT_LEAN_READS) == len(o) - 1


@pytest.mark.parametrize("debug", [True, False])
def test_single_end(root, oracle_mod, debug):
    """single-end, an odd count, through the general kernel and the lean kernel"""
    idx = ec.index_for(root, 31, "dense")
    with _gpu(idx, debug=debug) as (qi, mp):
        for variant in ("default", "selAln"):
            idx, rd, rs, what = _ref(root, oracle_mod, 31, 100, "dense", variant, single=True)
            q, o = pack(ec.odd_single(rd["r1"], rd["r2"]))
            gs = mp.map_reads(q, o, opts=_gopts(variant, oracle_mod))
            ec.check(rs, gs, "%s, debug=%s" % (what, debug))
            if not debug:
                assert mp.stat(QM_STAT_LEAN_READS) == len(o) - 1


def test_packed_reads_and_stage_view(root, oracle_mod):
    """the reads sent 2-bit packed (map_pairs_packed) give the fused result; the stage entry points (map_pairs_stages, with and without
    intervals, reads as characters and packed) give it unit by unit but for the units whose excess orphans only the caller drops"""
    idx, rd, res, what = _ref(root, oracle_mod, 31, 100, "dense", "default")
    a = (rd["q1"], rd["o1"], rd["q2"], rd["o2"])
    with _gpu(idx, debug=False) as (qi, mp):
        fused = mp.map_pairs(*a)
        ec.check(res, fused, "fused, " + what)
        hits, offs, ctr = fused.hits.copy(), fused.hit_offsets.copy(), dict(fused.counters)
        gp = mp.map_pairs_packed(*a)
        assert np.array_equal(offs, gp.hit_offsets) and hits.tobytes() == gp.hits.tobytes() and ctr == gp.counters
        ec.check(res, gp, "packed pairs, " + what)
        full = mp.map_pairs_stages(*a)
        kc.check_stage_view(res, full, "stage view with intervals, " + what)
        for packed in (False, True):
            light = mp.map_pairs_stages(*a, no_intervals=True, packed=packed)
            assert mp.stat(QM_STAT_LEAN_READS) == 2 * rd["n"], "the lean / pair kernel did not run"
            kc.check_stage_view(res, light, "stage view without intervals, packed=%s, %s" % (packed, what))


@pytest.mark.parametrize("k", [31, 17])
def test_table_builders(root, oracle_mod, k, monkeypatch):
    """QM_TABLE_CHECK=1 holds every entry of SaExt / SaExt2 / sanext as the packed builders made it against the byte-per-character builders
    and fails the build on a difference -- on a text where a `$` follows many k-mers at once and the last k-mer ends the text: one -s call
    (sanext), one with 150-character reads (SaExt2), and one with 100-character reads on a fresh mapper (SaExt alone)"""
    monkeypatch.setenv("QM_TABLE_CHECK", "1")
    idx = ec.index_for(root, k, "dense")
    with _gpu(idx, debug=False, wide_reads=True) as (qi, mp):
        idx, rd, res, what = _ref(root, oracle_mod, k, 100, "dense", "selAln")
        gr = mp.map_pairs(rd["q1"], rd["o1"], rd["q2"], rd["o2"], opts=_gopts("selAln", oracle_mod))
        ec.check(res, gr, "checked tables, " + what)
        idx, rw, resw, what = _ref(root, oracle_mod, k, 150, "dense", "default")
        gw = mp.map_pairs(rw["q1"], rw["o1"], rw["q2"], rw["o2"])
        ec.check(resw, gw, "checked tables, " + what)
        assert mp.stat(QM_STAT_LEAN_READS) == 2 * rw["n"], "the wide lean kernel did not run: no SaExt2"
    with _gpu(idx, debug=False) as (qi, mp):
        idx, rd, res, what = _ref(root, oracle_mod, k, 100, "dense", "default")
        gr = mp.map_pairs(rd["q1"], rd["o1"], rd["q2"], rd["o2"])
        ec.check(res, gr, "checked tables, fresh mapper, " + what)
        assert mp.stat(QM_STAT_LEAN_READS) == 2 * rd["n"]


@pytest.mark.parametrize("kernel", ["general", "pair"])
def test_true_positions(root, oracle_mod, kernel):
    """ends_cases.truth_check on the DEVICE's hits: no oracle, no suffix array"""
    idx, rd, res, what = _ref(root, oracle_mod, 31, 100, "dense", "default")
    with _gpu(idx, debug=kernel == "general") as (qi, mp):
        gr = mp.map_pairs(rd["q1"], rd["o1"], rd["q2"], rd["o2"])
        assert mp.stat(QM_STAT_LEAN_READS) == (-1 if kernel == "general" else 2 * rd["n"])
        got = ec.truth_check(gr.hit_offsets, gr.hits, ec.covered(rd["truth"], 31))
        print("truth_check, %s kernel, %s: %d mates, %d with a negative position" % ((kernel, what) + got))
        q, o = pack(ec.odd_single(rd["r1"], rd["r2"]))
        gs = mp.map_reads(q, o)
        ec.truth_check(gs.hit_offsets, gs.hits, None, single=ec.covered_single(rd["truth"], 31))


def test_fragment_lengths(root, oracle_mod):
    """the device's histogram over the default mapping equals fld_cases' restatement over the oracle's hits; the effective lengths from it
    equal the restatement's for every transcript, the 1-, 5- and (k - 1)-character ones included"""
    import rapmap_amd as ra
    idx, rd, res, what = _ref(root, oracle_mod, 31, 100, "dense", "default")
    counts, st = fc.classify(res.hit_offsets, res.hits, 1000)
    with _gpu(idx, debug=False) as (qi, mp):
        mp.map_pairs(rd["q1"], rd["o1"], rd["q2"], rd["o2"])
        f = ra.FragLenDist(mp)
        try:
            f.add(mp)
            fc.assert_same(f.counts(), f.stat(), counts, st, what + ": the oracle's hits")
            print("fragment lengths, %s: %r" % (what, st))
            assert st["units"] == rd["n"] and st["used"] >= 100, st
            assert np.array_equal(qi.txp_lens, rd["lens"]) and rd["lens"].min() == 1 and (rd["lens"] == 5).any() and (rd["lens"] == 30).any()
            assert f.eff_lens(qi.txp_lens).tobytes() == fc.eff_lens(counts, qi.txp_lens).tobytes()
        finally:
            f.close()
