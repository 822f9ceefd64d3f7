"""What the oracle-parity mapping tests share -- the lane emulation (test_emu_parity, test_kmer_lengths, test_txp_ends, test_txp_repeats)
and the HIP path (their *_gpu twins, test_gpu_parity): the named option sets, the mapper and index of a GPU test as a context that closes
them, the process-wide caches of oracles, emulations and oracle results, the comparisons against the oracle, and the scenarios the
families run alike.

A family is a case module (ends_cases, repeat_cases) with index_for(root, k, image), reads_for(k, L) -- and, where its tests map a batch
with one longer pair behind it, mixed(k, L, extra) -- and optionally after_ref(res, rd, L, variant, what), called once on every oracle
result when it is computed.  Plain functions that take the family; no test functions here.  The asserts of this module are not rewritten
by pytest, so each carries its values in its message."""
import contextlib
import os
import time
import types

import numpy as np

from conftest import load_oracle
from util import assert_hits_equal, pack

# ---- the option sets: name -> (the oracle's spelling, the library's and the emulation's spelling); "mimic*": made by opts_for()

OPTION_SETS = {
    "default": ({}, {}),
    "noStrictCheck": ({"strictCheck": 0}, {"strict_check": 0}),
    "z0.9": ({"quasiCov": 0.9}, {"quasi_cov": 0.9}),
    "m3": ({"maxNumHits": 3}, {"max_num_hits": 3}),
    "noOrphans": ({"noOrphans": 1}, {"no_orphans": 1}),
    "noDovetail": ({"noDovetail": 1}, {"no_dovetail": 1}),
    "maxInterval50": ({"maxInterval": 50}, {"max_interval": 50}),
    "noSensitive": ({"sensitive": 0}, {"sensitive": 0}),
    "noSensitive_noStrict": ({"sensitive": 0, "strictCheck": 0}, {"sensitive": 0, "strict_check": 0}),
    "noSensitive_z0.8": ({"sensitive": 0, "quasiCov": 0.8}, {"sensitive": 0, "quasi_cov": 0.8}),
    "fuzzy": ({"fuzzy": 1}, {"fuzzy": 1}),
    "fuzzy_noOrphans_m3": ({"fuzzy": 1, "noOrphans": 1, "maxNumHits": 3}, {"fuzzy": 1, "no_orphans": 1, "max_num_hits": 3}),
    "fuzzy_noDovetail": ({"fuzzy": 1, "noDovetail": 1}, {"fuzzy": 1, "no_dovetail": 1}),
    "fuzzy_noSensitive": ({"fuzzy": 1, "sensitive": 0}, {"fuzzy": 1, "sensitive": 0}),
    "selAln": ({"selAln": 1}, {"sel_aln": 1}),
    "selAln_hardFilter": ({"selAln": 1, "hardFilter": 1}, {"sel_aln": 1, "hard_filter": 1}),
    "selAln_fullband": ({"selAln": 1, "dpBandwidth": -1}, {"sel_aln": 1, "dp_bandwidth": -1}),
    "mimicBT2": None,
    "mimicStrictBT2": None,
}
# every set of test_emu_parity.test_synth_small and test_gpu_parity.test_synth_small
PLAIN_SETS = ("default", "noStrictCheck", "z0.9", "m3", "noOrphans", "noDovetail", "maxInterval50", "noSensitive", "noSensitive_noStrict", "noSensitive_z0.8",
              "fuzzy", "fuzzy_noOrphans_m3", "fuzzy_noDovetail", "fuzzy_noSensitive")
HEADLINE_KERNELS = ["pair", "lean"]


def is_sel(variant):
    """selective alignment (-s): no SA-interval records to compare, and a status whose upper bits count the slow pass"""
    return variant.startswith("selAln") or variant.startswith("mimic")


def oracle_opts(variant, oracle_mod):
    if variant.startswith("mimic"):
        return oracle_mod.mimic_bt2_opts(strict=variant == "mimicStrictBT2")
    return oracle_mod.default_opts(**OPTION_SETS[variant][0])


def opts_for(variant, oracle_mod, default_opts):
    """(the oracle's options, the options of the code under test: default_opts is emu.default_opts or rapmap_amd.default_opts)"""
    if variant.startswith("mimic"):
        strict = variant == "mimicStrictBT2"
        mine = dict(sel_aln=1, aln_policy=2 if strict else 1, no_orphans=1, no_dovetail=1, consensus_slack=0.35, max_num_hits=1000)
        if strict:
            mine.update(min_score_fraction=0.8, match_score=1, mismatch_penalty=0, gap_open=25, gap_extend=25)
    else:
        mine = OPTION_SETS[variant][1]
    return oracle_opts(variant, oracle_mod), default_opts(**mine)


def lib_opts(variant, oracle_mod):
    import rapmap_amd as ra
    return opts_for(variant, oracle_mod, ra.default_opts)[1]


def emu_opts(variant, oracle_mod):
    import emu
    return opts_for(variant, oracle_mod, emu.default_opts)[1]


# ---- small helpers of the case modules

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.zeros(256, np.uint8)
COMP[:] = ord("N")
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    COMP[_a] = _b

_cache = {}


def once(key, make):
    """make(), once per process and key"""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def subdir(tmp_root, name):
    d = os.path.join(str(tmp_root), name)
    os.makedirs(d, exist_ok=True)
    return d


def build(fasta, out, k, image, threads=4):
    import rapmap_amd as ra
    assert image in ("dense", "ph"), image
    ra.build_index(fasta, out, k=k, threads=threads, perfect_hash=image == "ph")
    return out


def index_of(tmp_root, tag, k, image, names, seqs):
    """the transcripts written to <tmp_root>/<tag>_k<k>/txome.fa and indexed at k; image: "dense" or "ph" (`quasiindex -p`).  The index
    holds every transcript, in file order."""
    import rapmap_amd as ra
    from rapmap_amd import synth
    d = subdir(tmp_root, "%s_k%d" % (tag, k))
    fa = os.path.join(d, "txome.fa")
    if not os.path.exists(fa):
        synth.write_fasta(fa, names, seqs)
    idx = build(fa, os.path.join(d, "idx_%s" % image), k, image, threads=2)
    qi = ra.QuasiIndex(idx)
    try:
        assert qi.txp_names == names and [int(x) for x in qi.txp_lens] == [s.size for s in seqs], "the index does not hold the transcripts as written"
    finally:
        qi.close()
    return idx


def odd_single(r1, r2):
    """single-end reads, an odd count: mate 1 of every pair but the last, and one mate 2"""
    one = list(r1[:-1]) + list(r2[1:2])
    if len(one) % 2 == 0:
        one = one[:-1]
    return one


class Timer:
    """the line a test prints per group of device calls (on=False: nothing)"""
    def __init__(self, what, on=True):
        self.what, self.on, self.t0 = what, on, time.perf_counter()

    def done(self, calls):
        if self.on:
            print("%s: %d device calls, %.2f s" % (self.what, calls, time.perf_counter() - self.t0))


# ---- the code under test on the device

@contextlib.contextmanager
def gpu_mapper(idx, debug=True, ph_compact=False, pair_kernel=True, wide_reads=False):
    """(QuasiIndex, QuasiMapper) of an index, both closed on the way out.  debug=True keeps the SA-interval records of a fused call
    (qm_fetch_intervals) -- and so runs the GENERAL stage-A kernel; the kernels the headline is quoted on (the pair kernel,
    qm_lean_kernel) only run with debug=False: headline() below"""
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


def headline(idx, kernel, ph_compact=False):
    """a mapper whose paired calls run the pair kernel (qm_duo.inl) or qm_lean_kernel alone (QM_CTX_NO_PAIR_KERNEL)"""
    return gpu_mapper(idx, debug=False, ph_compact=ph_compact, pair_kernel=kernel == "pair")


# ---- caches, for the process: nothing kept here is ever changed

_oracles, _emus, _refs = {}, {}, {}


def oracle_of(idx):
    """(index as the oracle reads it, oracle)"""
    if idx not in _oracles:
        _oracles[idx] = load_oracle(idx)
    return _oracles[idx]


def emu_of(idx, image="dense"):
    """(index as the oracle reads it, oracle, emulation): the emulation's extension tables are built once per index.  image "ph": the -p
    index looked up through the bucket table the device flattens it into; otherwise a -p index is looked up through the emulated BooPHF
    levels and the membership filter (the device's compact image)"""
    import emu
    if (idx, image) not in _emus:
        ix, orc = oracle_of(idx)
        em = emu.Emu(ix)
        if image == "ph":
            assert em.ph, "not a -p index: " + idx
            em.ph = None
        _emus[(idx, image)] = (ix, orc, em)
    return _emus[(idx, image)]


def ref(fam, root, oracle_mod, k, L, image, variant, single=False, ints=False, extra=0):
    """the oracle's result of one configuration of a family, computed once and shared (never changed).  single: the units of
    odd_single(); extra: the pairs of reads_for(k, L) with one pair of `extra` characters behind them (fam.mixed); ints: with the
    SA-interval records.  -> .idx, .rd (the read set), .a (the packed reads of the call: (q1, o1, q2, o2) or (q, o)), .n (units), .res, .what"""
    idx = fam.index_for(root, k, "dense" if image == "dense" else "ph")
    rd = fam.reads_for(k, L)
    if single:
        a = pack(odd_single(rd["r1"], rd["r2"]))
        assert (len(a[1]) - 1) % 2 == 1, len(a[1]) - 1
    elif extra:
        a = fam.mixed(k, L, extra)
    else:
        a = (rd["q1"], rd["o1"], rd["q2"], rd["o2"])
    what = "k=%d L=%d%s %s %s%s" % (k, L, " + one pair of %d" % extra if extra else "", image, variant, ", single-end" if single else "")
    key = (idx, L, variant, single, ints, extra)
    if key not in _refs:
        orc, oopts = oracle_of(idx)[1], oracle_opts(variant, oracle_mod)
        res = orc.map_single(*a, opts=oopts, nthreads=8) if single else orc.map_pairs(*a, opts=oopts, nthreads=8, want_ints=ints)
        if hasattr(fam, "after_ref"):
            fam.after_ref(res, rd, L, variant, what)
        _refs[key] = res
    return types.SimpleNamespace(idx=idx, rd=rd, a=a, n=len(a[1]) - 1, res=_refs[key], what=what)


def emu_ref(fam, root, oracle_mod, k, L, image, variant, single=False):
    """ref() as the emulation tests ask for it: with the interval records where the call keeps them (paired, without -s)"""
    return ref(fam, root, oracle_mod, k, L, image, variant, single=single, ints=not single and not is_sel(variant))


# ---- the checks

INT_COLS = ((0, "begin"), (1, "end"), (2, "len"), (3, "query_pos"), (5, "list"))


def check_intervals(res, offs, recs, what=""):
    """the SA-interval records (offsets, records) of the code under test equal the oracle's (res mapped with want_ints=True), five columns"""
    assert np.array_equal(res.ints_offsets, offs), what + ": interval offsets"
    for col, name in INT_COLS:
        assert np.array_equal(res.ints[:, col], recs[name].astype(np.int32)), "%s: interval column %s" % (what, name)


def check(res, got, what, ints=None):
    """hits and counters of `got` (an emulation or a device result) equal the oracle's `res`; ints = (offsets, records) where the
    SA-interval records were kept: their five columns equal the oracle's too (res mapped with want_ints=True)"""
    assert_hits_equal(res.hit_offsets, res.hits, got.hit_offsets, got.hits, what)
    assert res.counters == got.counters, (what, res.counters, got.counters)
    if ints is not None:
        check_intervals(res, ints[0], ints[1], what)


def check_emu(res, er, what, ints=False):
    """check() of an emulation result, with its interval records where ints"""
    check(res, er, what, ints=(er.int_offsets, er.ints) if ints else None)


def status_ok(er, variant, what):
    """the emulation's own cross-checks found nothing.  -s: bits 8 and up count the reads of the slow pass, and some data sends many there"""
    assert (er.status & 0xff if is_sel(variant) else er.status) == 0, (what, er.status)


def check_stage_view(res, stage, what, max_num_hits=200):
    """The merge of a stage view (map_pairs_stages: stage B without the caller-level bookkeeping) against the oracle's fused result `res`
    under default options.  The one thing the caller's bookkeeping does there is drop the orphans of a unit that has more than maxNumHits
    of them (RapMapSAMapper.cpp:534-536; unit_merge's `merge_only`): such a unit is empty in `res` and keeps its orphans in the stage view.
    Every other unit's records equal the oracle's byte for byte; peHits, seHits, numReads and tooManyHits are the oracle's, totHits and
    mappedUnits are the oracle's plus what those units keep.  -> the number of such units"""
    so, ro = np.asarray(stage.hit_offsets), np.asarray(res.hit_offsets)
    assert so.size == ro.size, (what, so.size, ro.size)
    sc, rc = np.diff(so), np.diff(ro)
    differ = np.nonzero(sc != rc)[0]
    kept = 0
    for u in differ:
        h = stage.hits[so[u]:so[u + 1]]
        assert rc[u] == 0 and sc[u] > max_num_hits and not h["is_paired"].any() and (h["mate_status"] != 3).all(), \
            "%s: unit %d has %d hits in the stage view, %d in the fused result" % (what, u, sc[u], rc[u])
        kept += int(sc[u])
    same = np.repeat(sc == rc, sc)
    assert stage.hits[same].tobytes() == res.hits.tobytes(), what + ": hit records differ from the fused result"
    want = dict(res.counters)
    want["totHits"] += kept
    want["mappedUnits"] += len(differ)
    assert stage.counters == want, (what, stage.counters, want)
    return len(differ)


def check_headline(mp, kernel, n_pairs, expect_deferred=True, fuzzy=False, some_merged=True):
    """the call just made went through the kernel it was meant for, and that kernel decided to leave some reads to the general one"""
    import rapmap_amd as ra
    lean, deferred, pairs = mp.stat(ra.QM_STAT_LEAN_READS), mp.stat(ra.QM_STAT_LEAN_DEFERRED), mp.stat(ra.QM_STAT_PAIR_KERNEL_PAIRS)
    assert lean == 2 * n_pairs, "the lean / pair kernel did not run: QM_STAT_LEAN_READS %d, %d pairs" % (lean, n_pairs)
    assert (0 < deferred < 2 * n_pairs) if expect_deferred else deferred >= 0, deferred
    if kernel == "pair":
        assert pairs == n_pairs, (pairs, n_pairs)
        merged = mp.stat(ra.QM_STAT_PAIRS_MERGED)
        assert merged == 0 if fuzzy else (1 if some_merged else 0) <= merged <= n_pairs - (deferred + 1) // 2, (merged, deferred)
    else:
        assert pairs == -1, pairs
    return deferred


def same_result(a, hits, offs, ctr, what):
    """result `a` equals the copies (hits, offsets, counters) kept of an earlier one on the same mapper"""
    assert np.array_equal(offs, a.hit_offsets) and hits.tobytes() == a.hits.tobytes() and ctr == a.counters, (what, ctr, a.counters)


# ---- scenarios under the lane emulation

def emu_pairs(fam, root, oracle_mod, k, L, image, variant, ns=2, slow_pass_ok=False, note="", flat_ph=True):
    """one paired call through the oracle and the emulation -> (ref(), the emulation's result).  slow_pass_ok: -s may send reads to its
    slow pass (status_ok); otherwise the status is 0.  flat_ph: image "ph" is looked up through the flattened bucket table (emu_of), any
    other image of a -p index through the BooPHF levels"""
    r = emu_ref(fam, root, oracle_mod, k, L, image, variant)
    what = r.what + note
    er = emu_of(r.idx, "ph" if flat_ph and image == "ph" else "dense")[2].map(*r.a, opts=emu_opts(variant, oracle_mod), ns=ns)
    if slow_pass_ok:
        status_ok(er, variant, what)
    else:
        assert er.status == 0, (what, er.status)
    check_emu(r.res, er, what, ints=not is_sel(variant))
    return r, er


def emu_single_end(fam, root, oracle_mod, k, L, variant, ns, slow_pass_ok=False, note=""):
    """single-end, an odd count, through the oracle and the emulation"""
    r = emu_ref(fam, root, oracle_mod, k, L, "dense", variant, single=True)
    er = emu_of(r.idx)[2].map(*r.a, opts=emu_opts(variant, oracle_mod), ns=ns)
    if slow_pass_ok:
        status_ok(er, variant, r.what)
    else:
        assert er.status == 0, (r.what, er.status)
    check(r.res, er, r.what + note)


# ---- scenarios on the device.  timed: print a Timer line; lean_sets: the option sets under which QM_STAT_LEAN_READS is held to the
# number of reads of the call

def general_kernel(fam, root, oracle_mod, k, L, image, variants, ph_compact=False, timed=False):
    """the general stage-A kernel (intervals kept): hits, counters and, where -s is off, the interval lists"""
    import rapmap_amd as ra
    with gpu_mapper(fam.index_for(root, k, image), debug=True, ph_compact=ph_compact) as (qi, mp):
        assert qi.perfect_hash == (image == "ph"), (qi.perfect_hash, image)
        for variant in variants:
            ints = not is_sel(variant)
            r = ref(fam, root, oracle_mod, k, L, image, variant, ints=ints)
            tm = Timer("general kernel, " + r.what + (", compact" if ph_compact else ""), timed)
            gr = mp.map_pairs(*r.a, opts=lib_opts(variant, oracle_mod))
            if ints:                                     # (with -s the lean kernel's collector edition writes the interval records itself)
                assert mp.stat(ra.QM_STAT_LEAN_READS) == -1, "expected the general kernel: QM_STAT_LEAN_READS %d" % mp.stat(ra.QM_STAT_LEAN_READS)
            check(r.res, gr, tm.what, ints=mp.intervals(r.n) if ints else None)
            tm.done(1)


def lean_kernel_compact_ph(fam, root, oracle_mod, k, lean_sets, expect_left=None, timed=False):
    """the compact -p image, where the host launches qm_lean_kernel's PH edition.  expect_left: the reads it leaves under default options"""
    import rapmap_amd as ra
    with gpu_mapper(fam.index_for(root, k, "ph"), debug=False, ph_compact=True) as (qi, mp):
        assert qi.perfect_hash
        for variant in ("default", "selAln"):
            r = ref(fam, root, oracle_mod, k, 100, "ph", variant)
            tm = Timer("lean kernel, compact -p, " + r.what, timed)
            gr = mp.map_pairs(*r.a, opts=lib_opts(variant, oracle_mod))
            check(r.res, gr, tm.what)
            tm.done(1)
            if variant in lean_sets:
                assert mp.stat(ra.QM_STAT_LEAN_READS) == 2 * r.n, "the lean kernel did not run: QM_STAT_LEAN_READS %d" % mp.stat(ra.QM_STAT_LEAN_READS)
            if variant == "default" and expect_left is not None:
                assert mp.stat(ra.QM_STAT_LEAN_DEFERRED) == expect_left, (mp.stat(ra.QM_STAT_LEAN_DEFERRED), expect_left)


def wide_lean_kernel(fam, root, oracle_mod, k, L, slow_pass=False, timed=False):
    """reads beyond 128 characters: the wide lean kernel (one read per wavefront), default and -s, paired and single-end.  slow_pass: the
    data sends reads to the slow pass of -s, and the test says how many"""
    import rapmap_amd as ra
    with gpu_mapper(fam.index_for(root, k, "dense"), debug=False) as (qi, mp):
        tm = Timer("wide lean kernel, L=%d" % L, timed)
        for variant in ("default", "selAln"):
            r = ref(fam, root, oracle_mod, k, L, "dense", variant)
            gr = mp.map_pairs(*r.a, opts=lib_opts(variant, oracle_mod))
            check(r.res, gr, "wide lean kernel, " + r.what)
            if variant == "default":
                assert mp.stat(ra.QM_STAT_LEAN_READS) == 2 * r.n, "the wide lean kernel did not run: no SaExt2 (QM_STAT_LEAN_READS %d)" % mp.stat(ra.QM_STAT_LEAN_READS)
            elif slow_pass:
                slow = mp.stat(ra.QM_STAT_SLOW_READS)
                print("wide lean kernel, %s: %d reads on the slow path of -s" % (r.what, slow))
                assert slow > 0, slow
            r = ref(fam, root, oracle_mod, k, L, "dense", variant, single=True)
            gs = mp.map_reads(*r.a, opts=lib_opts(variant, oracle_mod))
            check(r.res, gs, "wide lean kernel, " + r.what)
            if variant == "default":
                assert mp.stat(ra.QM_STAT_LEAN_READS) == r.n, (mp.stat(ra.QM_STAT_LEAN_READS), r.n)
        tm.done(4)


def single_end(fam, root, oracle_mod, debug, lean_sets, timed=False):
    """single-end, an odd count, through the general kernel (debug) and the lean kernel"""
    import rapmap_amd as ra
    with gpu_mapper(fam.index_for(root, 31, "dense"), debug=debug) as (qi, mp):
        tm = Timer("single-end, debug=%s" % debug, timed)
        for variant in ("default", "selAln"):
            r = ref(fam, root, oracle_mod, 31, 100, "dense", variant, single=True)
            gs = mp.map_reads(*r.a, opts=lib_opts(variant, oracle_mod))
            check(r.res, gs, "%s, debug=%s" % (r.what, debug))
            if not debug and variant in lean_sets:
                assert mp.stat(ra.QM_STAT_LEAN_READS) == r.n, (mp.stat(ra.QM_STAT_LEAN_READS), r.n)
        tm.done(2)


def packed_reads_and_stage_view(fam, root, oracle_mod, expect_left=None, timed=False):
    """the reads sent 2-bit packed (map_pairs_packed) give the fused result; the stage entry points (map_pairs_stages, with and without
    intervals, reads as characters and packed) give it unit by unit but for the units whose excess orphans only the caller drops.
    expect_left: the reads the pair kernel leaves in the stage view without intervals"""
    import rapmap_amd as ra
    r = ref(fam, root, oracle_mod, 31, 100, "dense", "default")
    with gpu_mapper(r.idx, debug=False) as (qi, mp):
        tm = Timer("packed reads and stage view, " + r.what, timed)
        fused = mp.map_pairs(*r.a)
        check(r.res, fused, "fused, " + r.what)
        hits, offs, ctr = fused.hits.copy(), fused.hit_offsets.copy(), dict(fused.counters)
        gp = mp.map_pairs_packed(*r.a)
        same_result(gp, hits, offs, ctr, "packed pairs against fused, " + r.what)
        check(r.res, gp, "packed pairs, " + r.what)
        full = mp.map_pairs_stages(*r.a)
        check_stage_view(r.res, full, "stage view with intervals, " + r.what)
        for packed in (False, True):
            light = mp.map_pairs_stages(*r.a, no_intervals=True, packed=packed)
            assert mp.stat(ra.QM_STAT_LEAN_READS) == 2 * r.n, "the lean / pair kernel did not run: QM_STAT_LEAN_READS %d" % mp.stat(ra.QM_STAT_LEAN_READS)
            if expect_left is not None:
                assert mp.stat(ra.QM_STAT_LEAN_DEFERRED) == expect_left, (mp.stat(ra.QM_STAT_LEAN_DEFERRED), expect_left)
            check_stage_view(r.res, light, "stage view without intervals, packed=%s, %s" % (packed, r.what))
        tm.done(5)


def table_builders(fam, root, oracle_mod, k, timed=False):
    """with QM_TABLE_CHECK=1 set by the test: one -s call (sanext), one with 150-character reads (SaExt2), and one with 100-character reads
    on a fresh mapper (SaExt alone)"""
    import rapmap_amd as ra
    idx = fam.index_for(root, k, "dense")
    tm = Timer("checked tables", timed)
    with gpu_mapper(idx, debug=False, wide_reads=True) as (qi, mp):
        r = ref(fam, root, oracle_mod, k, 100, "dense", "selAln")
        check(r.res, mp.map_pairs(*r.a, opts=lib_opts("selAln", oracle_mod)), "checked tables, " + r.what)
        r = ref(fam, root, oracle_mod, k, 150, "dense", "default")
        check(r.res, mp.map_pairs(*r.a), "checked tables, " + r.what)
        assert mp.stat(ra.QM_STAT_LEAN_READS) == 2 * r.n, "the wide lean kernel did not run: no SaExt2 (QM_STAT_LEAN_READS %d)" % mp.stat(ra.QM_STAT_LEAN_READS)
    with gpu_mapper(idx, debug=False) as (qi, mp):
        r = ref(fam, root, oracle_mod, k, 100, "dense", "default")
        check(r.res, mp.map_pairs(*r.a), "checked tables, fresh mapper, " + r.what)
        assert mp.stat(ra.QM_STAT_LEAN_READS) == 2 * r.n, (mp.stat(ra.QM_STAT_LEAN_READS), r.n)
    tm.done(3)


def fragment_lengths(fam, root, oracle_mod, timed=False):
    """the device's histogram over the default mapping equals fld_cases' restatement over the oracle's hits, and the effective lengths
    from it equal the restatement's for every transcript -> ref()"""
    import fld_cases as fc
    import rapmap_amd as ra
    r = ref(fam, root, oracle_mod, 31, 100, "dense", "default")
    counts, st = fc.classify(r.res.hit_offsets, r.res.hits, 1000)
    with gpu_mapper(r.idx, debug=False) as (qi, mp):
        tm = Timer("fragment lengths, " + r.what, timed)
        mp.map_pairs(*r.a)
        f = ra.FragLenDist(mp)
        try:
            f.add(mp)
            fc.assert_same(f.counts(), f.stat(), counts, st, r.what + ": the oracle's hits")
            print("fragment lengths, %s: %r" % (r.what, st))
            assert st["units"] == r.n and st["used"] >= 100, st
            assert np.array_equal(qi.txp_lens, r.rd["lens"]), "the index's transcript lengths are not the read set's"
            assert f.eff_lens(qi.txp_lens).tobytes() == fc.eff_lens(counts, qi.txp_lens).tobytes(), r.what + ": effective lengths"
        finally:
            f.close()
        tm.done(1)
    return r
