"""Many trips per wavefront, the part that needs no GPU (tile_cases.py; the device runs in test_many_trips_gpu.py, -m gpu).

  - tile_cases.expected() is held to the ORACLE mapping a tiled batch itself: the one proof that gathering the base result by the
    permutation is right, so it goes through nothing under test.
  - The tiled batches put the kinds of reads that dirty a wavefront's state in front of the kinds that would show it (the `neighbours`
    condition), for every leg of the GPU module on a whole device of 256 compute units.
  - The answer does not depend on the order of the reads: one shuffled copy through the lane emulation of every stage-A kernel.  (The
    emulation runs three waves over a batch, thousands of trips each, so it has always covered the loops' logic; what it cannot show
    -- a missing wait on the LDS DMA, a fence -- is the device module's.)"""
import numpy as np
import pytest

import kmer_cases as kc
import mapping_harness as mh
import tile_cases as tc

KERNELS = {"pair": {}, "lean": {"QM_EMU_NO_DUO": "1"}, "general": {"QM_EMU_NO_LEAN": "1", "QM_EMU_NO_DUO": "1"}}


@pytest.fixture(scope="module")
def root(tmp_path_factory, lib_built, oracle_mod):
    yield tmp_path_factory.mktemp("many_trips")
    tc.forget_tiles()


def test_tile_moves_whole_units():
    """tile() on a batch small enough to check read by read: both mates of a pair move together, every base unit stands `copies` times"""
    r1 = [b"ACGT", b"", b"GGGTTTAAA", b"C", b"TTNTT"]
    r2 = [b"T", b"CCCC", b"", b"GATTACA", b"AC"]
    from util import pack
    a = pack(r1) + pack(r2)
    t, perm = tc.tile(a, 3, 7)
    assert sorted(perm.tolist()) == sorted(list(range(5)) * 3) and perm.tolist() != (list(range(5)) * 3)
    for i, u in enumerate(perm):
        assert t[0][t[1][i]:t[1][i + 1]].tobytes() == r1[u] and t[2][t[3][i]:t[3][i + 1]].tobytes() == r2[u], (i, u)
    assert t[1][-1] == t[0].size == 3 * sum(map(len, r1)) and t[3][-1] == t[2].size == 3 * sum(map(len, r2))
    assert np.array_equal(tc.tile(a, 3, 7)[1], perm) and not np.array_equal(tc.tile(a, 3, 8)[1], perm)


@pytest.mark.parametrize("variant", ["default", "selAln"])
@pytest.mark.parametrize("single", [False, True], ids=["paired", "odd_single"])
def test_helper_held_to_the_oracle(root, oracle_mod, variant, single):
    """600 units of golden synth_small, three shuffled copies: the ORACLE's result of the tiled batch equals expected() of its result of
    the base batch bit for bit -- hits, offsets, counters and, where it keeps them (paired), the interval records"""
    ints = not single
    b = tc.base("golden", root, oracle_mod, 31, 100, "dense", variant, single=single, ints=ints, limit=600)
    assert b.n == (599 if single else 600), b.n
    a, perm = tc.tile(b.a, 3, 11)
    want = tc.expected(b.res, perm, 3, ints=ints)
    orc, oopts = mh.oracle_of(b.idx)[1], mh.oracle_opts(variant, oracle_mod)
    got = orc.map_single(*a, opts=oopts, nthreads=8) if single else orc.map_pairs(*a, opts=oopts, nthreads=8, want_ints=True)
    assert len(got.hits) > 3 * 600, len(got.hits)
    mh.check(want, got, "the oracle on the tiled batch, " + b.what)
    if ints:
        assert np.array_equal(want.ints_offsets, got.ints_offsets) and want.ints.tobytes() == got.ints.tobytes(), b.what + ": interval records"
        assert len(got.ints) > 3 * 600, len(got.ints)


def test_widest_grids_and_copies():
    """the table of the issue on 256 compute units, as literals: 65 536 wavefronts for the pair and the lean kernel, 32 768 for -s and the
    general kernel, 98 304 on the compact image, 8 192 for the N-aware pass; six trips of each over the golden reads"""
    assert [tc.widest_waves("pair", 256), tc.widest_waves("lean", 256), tc.widest_waves("lean", 256, sel=True), tc.widest_waves("general", 256)] == [65536, 65536, 32768, 32768]
    assert [tc.widest_waves("pair", 256, compact=True), tc.widest_waves("lean", 256, compact=True), tc.widest_waves("general", 256, compact=True), tc.widest_waves("lean_nq", 256)] == [98304, 98304, 98304, 8192]
    assert tc.widest_waves("lean", 256, smallest=True) == 1024 and tc.widest_waves("lean", 32) == 8192
    # 4 234 pairs: 93 copies are 393 762 pairs >= 6 x 65 536 = 393 216, 92 are 389 528
    assert tc.copies_for("pair", 4234, 256) == 93 and tc.copies_for("lean", 4234, 256) == 93
    assert tc.trips_per_wave("pair", 93 * 4234, True, 65536) == (6, 7) and tc.trips_per_wave("pair", 92 * 4234, True, 65536) == (5, 6)
    # the general kernel a read per trip: 6 x 32 768 reads are 98 304 pairs; the wide lean kernel: 6 x 65 536 reads
    assert tc.copies_for("general", 4234, 256) == 24 and tc.copies_for("lean", 3000, 256, wide=True) == 66
    # single-end, two reads per trip: 6 x 65 536 x 2 = 786 432 reads
    assert tc.copies_for("lean", 4233, 256, paired=False) == 186
    assert tc.copies_for("lean", 4234, 256, compact=True) == 140 and 140 * 4234 < tc.MAX_UNITS


@pytest.mark.parametrize("leg", tc.LEGS, ids=lambda l: l.id)
def test_neighbours(root, oracle_mod, leg):
    """on 256 compute units, in every leg's tiled batch, the successive items of one wavefront hold at least 100 times each: a read with
    an N or another odd character, then a clean read that maps; a read with an interval of 64 suffixes or more, then one without a hit; a
    read of more than 100 characters, then one shorter than k.  (64 suffixes: the repeats family, whose arrays give them, and the golden
    transcriptome at k = 15 and 21; at k = 31 it and the ends family hold no k-mer that often, which is asserted.  Single-end calls keep
    no interval records.)"""
    b = tc.base(leg.fam, root, oracle_mod, leg.k, leg.L, "dense", "default", single=leg.single, ints=leg.paired)
    has_many = leg.fam == "repeats" or leg.k < 31
    kd = tc.kinds_of(leg.fam, root, oracle_mod, leg.k, leg.L, single=leg.single)
    assert bool(kd["many"].any()) == (has_many and leg.paired), "%s k=%d: are there intervals of 64 suffixes?  If so the combination applies" % (leg.fam, leg.k)
    if tc.per_read(leg.kernel, leg.paired, leg.wide):            # one read per wavefront and trip: a wavefront meets one mate only
        kd = tc.kinds_of(leg.fam, root, oracle_mod, leg.k, leg.L, per_mate=True)
    combos = [c for c in tc.COMBOS if c[0] != "many" or (has_many and leg.paired)]
    for variant in leg.variants:
        copies, nw = tc.leg_copies(leg, variant, b.n, 256)
        assert copies * b.n < tc.MAX_UNITS, (copies, b.n)
        stride = tc.unit_stride(leg.kernel, nw, leg.paired, leg.wide)
        got = tc.neighbours(tc.permutation(b.n, copies, tc.SEED), stride, kd, combos)
        print("%s %s: %d copies of %d units, stride %d units: %r" % (leg.id, variant, copies, b.n, stride, got))
        assert all(v >= tc.AT_LEAST for v in got.values()), (leg.id, variant, got)


def _emu_left(b, a, opts, capfd, kernels):
    """one emulated call -> (result, what the pair / lean kernel left under QM_EMU_LEAN_STATS)"""
    capfd.readouterr()
    er = mh.emu_of(b.idx)[2].map(*a, opts=opts, ns=2)
    left = kc.emu_left(capfd.readouterr().err)
    return er, {"pair": left.get("pair"), "lean": left.get("lean_first_pass", left.get("lean"))}.get(kernels)


@pytest.mark.parametrize("variant", ["default", "selAln"])
@pytest.mark.parametrize("kernels", sorted(KERNELS))
@pytest.mark.parametrize("fam", ["golden", "repeats"])
def test_order_independence_under_the_emulation(root, oracle_mod, fam, kernels, variant, capfd, monkeypatch):
    """one shuffled copy of a base batch through the emulated pair kernel, qm_lean_kernel alone and the general kernel alone: the oracle's
    result gathered by the permutation, the emulation's own cross-checks silent, and as many reads left to the general kernel as in the
    order the family wrote them"""
    for name, v in KERNELS[kernels].items():
        monkeypatch.setenv(name, v)
    monkeypatch.setenv("QM_EMU_LEAN_STATS", "1")
    ints = not mh.is_sel(variant)
    b = tc.base(fam, root, oracle_mod, 31, 100, "dense", variant, ints=ints)
    a, want, perm = tc.tiled(b, 1, tc.SEED, ints=ints)
    assert not np.array_equal(perm, np.arange(b.n))
    opts = mh.emu_opts(variant, oracle_mod)
    er, left = _emu_left(b, a, opts, capfd, kernels)
    what = "%s, one shuffled copy, %s kernel" % (b.what, kernels)
    mh.status_ok(er, variant, what)
    mh.check_emu(want, er, what, ints=ints)
    if variant == "default" and kernels != "general":
        er0, left0 = _emu_left(b, b.a, opts, capfd, kernels)
        mh.check_emu(b.res, er0, what + ", in the family's order", ints=ints)
        print("%s: the %s kernel left %r reads, %r in the family's order" % (what, kernels, left, left0))
        assert left is not None and 0 < left < 2 * b.n and left == left0, (left, left0)
