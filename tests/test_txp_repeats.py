"""Transcripts that repeat inside themselves (repeat_cases.py: tandem arrays, a dispersed segment, inverted repeats), through the device
mapper's source under the lane emulation (tests/emu), against the oracle: bit-exact hits, offsets, counters and SA-interval lists, and
`status == 0` (the emulation's own cross-checks of the pair, lean and packed kernels against the general one).  The same data runs on
the HIP path in test_txp_repeats_gpu.py (-m gpu).

What this reaches and nothing else does: an interval that lists one transcript more than once, so that "one position per transcript, the
smallest signed pos - queryPos" has something to choose between -- in single_interval_small, single_interval (staged and sainfo
branch), multi_interval (qm_mapper.inl), the lane reads over the parked suffixes of qm_lean.inl and qm_duo.inl, and the position lists
of -s (qm_sel.inl, qm_selpack.inl).  Reads of 100 characters are also mapped in the slot classes of longer reads (ns = 3, 4, 8: what the
host picks when a batch holds a longer read), where the staging of a first interval's records reaches beyond 64 suffixes."""
import pytest

import kmer_cases as kc
import mapping_harness as mh
import repeat_cases as rc

SLOT_SETS = ("default", "fuzzy", "noSensitive", "noDovetail", "m3", "maxInterval50", "selAln")
KERNELS = {"host": {}, "no_pair": {"QM_EMU_NO_DUO": "1"}, "general": {"QM_EMU_NO_LEAN": "1", "QM_EMU_NO_DUO": "1"}}


@pytest.fixture(scope="module")
def root(tmp_path_factory, lib_built, oracle_mod):
    return tmp_path_factory.mktemp("txp_repeats")


def _run(root, oracle_mod, k, L, image, variant, ns=2, kernels="host", monkeypatch=None):
    """one paired call through the oracle and the emulation"""
    for name, v in KERNELS[kernels].items():
        monkeypatch.setenv(name, v)
    r, er = mh.emu_pairs(rc, root, oracle_mod, k, L, image, variant, ns=ns, slow_pass_ok=True, note=" ns=%d %s" % (ns, kernels))
    print("%s ns=%d %s: %d pairs, %d hits, %r%s" % (r.what, ns, kernels, r.n, len(r.res.hits), r.res.counters,
                                                   ", %d reads on the slow pass of -s" % (er.status >> 8) if er.status >> 8 else ""))


@pytest.mark.parametrize("kernels", sorted(KERNELS))
@pytest.mark.parametrize("variant", rc.VARIANTS)
def test_pairs_k31(root, oracle_mod, variant, kernels, monkeypatch):
    """2 x 100 at k = 31, every option set; the kernels as the host would run them, without the pair kernel, the general kernel alone"""
    _run(root, oracle_mod, 31, 100, "dense", variant, kernels=kernels, monkeypatch=monkeypatch)


@pytest.mark.parametrize("variant", rc.FEW)
@pytest.mark.parametrize("k,image", [(15, "dense"), (21, "dense"), (31, "ph"), (31, "ph_compact")])
def test_pairs_other_k_and_images(root, oracle_mod, k, image, variant, monkeypatch):
    """k = 15 and 21 (the unit lengths k - 1, k, k + 1 move with k), and a -p index both ways the device holds it"""
    _run(root, oracle_mod, k, 100, image, variant, monkeypatch=monkeypatch)


@pytest.mark.parametrize("variant", SLOT_SETS)
@pytest.mark.parametrize("ns", [3, 4, 8])
def test_short_reads_in_the_slot_class_of_longer_ones(root, oracle_mod, ns, variant, monkeypatch):
    """reads of 100 characters at ns = 3, 4 and 8: the slots of the interval table behind the read's last k-mer then hold more than 64
    staged (tid, pos) records, and single_interval has to read every one of them"""
    _run(root, oracle_mod, 31, 100, "dense", variant, ns=ns, monkeypatch=monkeypatch)


@pytest.mark.parametrize("variant", ["default", "fuzzy", "selAln"])
@pytest.mark.parametrize("extra,ns", [(150, 3), (250, 4), (300, 8), (600, 2)])
def test_one_longer_pair_in_the_batch(root, oracle_mod, extra, ns, variant):
    """the batch as the device meets it: the pairs of 100 characters and one pair of 150, 250 or 300 behind them, in the slot class the
    host picks for the longest read; with a pair of 600 the others stay at ns = 2 and that pair goes through the long-read pass"""
    ints = not mh.is_sel(variant)
    r = mh.ref(rc, root, oracle_mod, 31, 100, "dense", variant, ints=ints, extra=extra)
    res = r.res
    er = mh.emu_of(r.idx)[2].map(*r.a, opts=mh.emu_opts(variant, oracle_mod), ns=ns)
    what = "k=31 L=100 + one pair of %d, %s ns=%d" % (extra, variant, ns)
    if extra > 512 and ints:
        assert er.status == 2 << 8, (what, er.status)        # (bits 8 and up: the two reads of the long-read pass)
    else:
        mh.status_ok(er, variant, what)
    mh.check_emu(res, er, what, ints=ints)
    assert res.hit_offsets[-1] > res.hit_offsets[-2], "the long pair did not map"


@pytest.mark.parametrize("variant", rc.FEW)
@pytest.mark.parametrize("L,ns", [(64, 2), (150, 3), (150, 4), (150, 8), (250, 4), (250, 8)])
def test_other_read_lengths(root, oracle_mod, L, ns, variant, monkeypatch):
    """reads of 150 and 250 characters in their own slot class (with the wide lean kernel held against the general one) and in wider ones;
    reads of 64 characters at ns = 2, where 64 NS - P is 94: the one way to more than 64 staged records in the narrowest class"""
    _run(root, oracle_mod, 31, L, "dense", variant, ns=ns, monkeypatch=monkeypatch)


@pytest.mark.parametrize("variant", ["default", "selAln"])
@pytest.mark.parametrize("k,L,ns", [(31, 100, 2), (31, 100, 3), (31, 100, 4), (31, 100, 8), (21, 150, 3), (31, 250, 4)])
def test_single_end(root, oracle_mod, k, L, ns, variant):
    """single-end, an odd count: the raw negative positions of the reads that hang over a transcript's start"""
    mh.emu_single_end(rc, root, oracle_mod, k, L, variant, ns, slow_pass_ok=True, note=" ns=%d" % ns)


@pytest.mark.parametrize("k,image", [(31, "dense"), (31, "ph_compact"), (21, "dense"), (15, "dense")])
def test_what_the_pair_and_lean_kernels_leave(root, oracle_mod, k, image, capfd, monkeypatch):
    """the reads the pair and the lean kernel leave are pinned, and among the reads they KEEP there are reads whose hit list comes from one
    interval that lists a transcript more than once: their per-transcript minimum over the parked suffixes had to choose"""
    r = mh.emu_ref(rc, root, oracle_mod, k, 100, image, "default")
    idx, rd, res, what = r.idx, r.rd, r.res, r.what
    monkeypatch.setenv("QM_EMU_LEAN_STATS", "2")
    capfd.readouterr()
    er = mh.emu_of(idx, image)[2].map(*r.a)
    err = capfd.readouterr().err
    assert er.status == 0
    left, which = kc.emu_left(err), rc.emu_left_reads(err)
    assert len(which["pair"]) == left["pair"] and len(which["lean"]) == left["lean"]
    rep = rc.reads_with_repeated_interval(mh.oracle_of(idx)[0], res)
    got = {"pair": left["pair"], "lean": left["lean"]}
    for name in ("pair", "lean"):
        kept = rep.copy()
        kept[sorted(which[name])] = False
        got[name + "_kept_repeated"] = int(kept.sum())
    print("%s: of %d reads (%d with a repeated interval) the emulation's pair / lean kernels left and kept %r" % (what, 2 * rd["n"], int(rep.sum()), got))
    assert got["pair_kept_repeated"] > 0 and got["lean_kept_repeated"] > 0, got
    assert got == rc.EXPECT_LEFT[(k, image)], (k, image, got)


@pytest.mark.parametrize("k,L", [(31, 100), (21, 100), (15, 100), (31, 150), (31, 250)])
def test_the_data_reaches_the_repeats(root, oracle_mod, k, L):
    """repeat_cases.reach on the oracle alone: negative positions, intervals that list a transcript twice in every width the code
    distinguishes, intervals beyond maxInterval 50 and 1000; the counts are pinned"""
    ix, orc = mh.oracle_of(rc.index_for(root, k, "dense"))
    got = rc.reach(ix, orc, oracle_mod, rc.reads_for(k, L), L, k)
    print("reach, k=%d L=%d: negative single-end %d, negative orphans %d, repeated intervals <= 64 / <= pfcap(3) / above: %d / %d / %d, intervals >= 50: %d, >= 1000: %d" % ((k, L) + got))
    rc.assert_reach(got, "k=%d L=%d" % (k, L), rc.pfcap(3, L, k))
    assert got == rc.REACH[(k, L)], got


@pytest.mark.parametrize("L", [100, 150, 250])
def test_oracle_holds_the_leftmost_positions(root, oracle_mod, L):
    """repeat_cases.truth_check on the ORACLE's hits, paired and single-end: the reference of every comparison here reports each covered
    mate on its own transcript at the leftmost place its characters occur there (and so does the emulation, which equals it)"""
    tx = rc.txome(31)
    r = mh.emu_ref(rc, root, oracle_mod, 31, L, "dense", "default")
    got = rc.truth_check(r.res.hit_offsets, r.res.hits, r.rd, tx, 31)
    print("truth_check, %s: %d eligible mates, %d checked, %d at a negative position, left out %r" % ((r.what,) + got))
    r = mh.emu_ref(rc, root, oracle_mod, 31, L, "dense", "default", single=True)
    got = rc.truth_check(r.res.hit_offsets, r.res.hits, r.rd, tx, 31, single=True)
    print("truth_check, %s: %d eligible mates, %d checked, %d at a negative position, left out %r" % ((r.what,) + got))
