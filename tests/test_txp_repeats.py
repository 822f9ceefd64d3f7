"""Transcripts that repeat inside themselves (repeat_cases.py: tandem arrays, a dispersed segment, inverted repeats), through the device
mapper's source under the lane emulation (tests/emu), against the oracle: bit-exact hits, offsets, counters and SA-interval lists, and
`status == 0` (the emulation's own cross-checks of the pair, lean and packed kernels against the general one).  The same data runs on
the HIP path in test_txp_repeats_gpu.py (-m gpu).

What this reaches and nothing else does: an interval that lists one transcript more than once, so that "one position per transcript, the
smallest signed pos - queryPos" has something to choose between -- in single_interval_small, single_interval (staged and sainfo
branch), multi_interval (qm_mapper.inl), the lane reads over the parked suffixes of qm_lean.inl and qm_duo.inl, and the position lists
of -s (qm_sel.inl, qm_selpack.inl).  Reads of 100 characters are also mapped in the slot classes of longer reads (ns = 3, 4, 8: what the
host picks when a batch holds a longer read), where the staging of a first interval's records reaches beyond 64 suffixes."""
import numpy as np
import pytest

import repeat_cases as rc
from conftest import load_oracle
from util import pack

_emus, _refs = {}, {}

# Reads the pair and the lean kernel leave to the general kernel on reads_for(k, 100) under default options, and how many of the reads
# they KEEP have their hit list from one interval that lists a transcript more than once (so their per-transcript minimum decided
# something).  From the lane emulation (QM_EMU_LEAN_STATS=2); test_txp_repeats_gpu.py holds qm_ctx_stat(QM_STAT_LEAN_DEFERRED) to
# "pair" / "lean".
EXPECT_LEFT = {
    (31, "dense"): {"pair": 2777, "lean": 1816, "pair_kept_repeated": 759, "lean_kept_repeated": 1582},
    (31, "ph_compact"): {"pair": 2777, "lean": 1816, "pair_kept_repeated": 759, "lean_kept_repeated": 1582},
    (21, "dense"): {"pair": 2976, "lean": 1944, "pair_kept_repeated": 720, "lean_kept_repeated": 1558},
    (15, "dense"): {"pair": 3300, "lean": 2247, "pair_kept_repeated": 613, "lean_kept_repeated": 1453},
}

SLOT_SETS = ("default", "fuzzy", "noSensitive", "noDovetail", "m3", "maxInterval50", "selAln")
KERNELS = {"host": {}, "no_pair": {"QM_EMU_NO_DUO": "1"}, "general": {"QM_EMU_NO_LEAN": "1", "QM_EMU_NO_DUO": "1"}}


def _emu(idx, image="dense"):
    """(index as the oracle reads it, oracle, emulation) of an index, kept for the process.  image "ph": the -p index looked up through
    the bucket table the device flattens it into; "ph_compact": through the emulated BooPHF levels and the membership filter"""
    import emu
    if (idx, image) not in _emus:
        ix, orc = _emus[(idx, "dense")][:2] if (idx, "dense") in _emus else load_oracle(idx)
        em = emu.Emu(ix)
        if image == "ph":
            assert em.ph
            em.ph = None
        _emus[(idx, image)] = (ix, orc, em)
    return _emus[(idx, image)]


@pytest.fixture(scope="module")
def root(tmp_path_factory, lib_built, oracle_mod):
    return tmp_path_factory.mktemp("txp_repeats")


def _index(root, k, image):
    return rc.index_for(root, k, "dense" if image == "dense" else "ph")


def _ref(root, oracle_mod, k, L, image, variant, single=False):
    """the oracle's result of one configuration, computed once and shared (never changed) -> (idx, read set, result, keeps intervals?, what)"""
    key = (k, L, image != "dense", variant, single)
    idx = _index(root, k, image)
    rd = rc.reads_for(k, L)
    if key not in _refs:
        import emu
        ix, orc, em = _emu(idx)
        oopts, _ = rc.opts_for(variant, oracle_mod, emu.default_opts)
        ints = not single and oopts.selAln == 0
        if single:
            q, o = pack(rc.odd_single(rd["r1"], rd["r2"]))
            assert (len(o) - 1) % 2 == 1
            res = orc.map_single(q, o, opts=oopts, nthreads=4)
        else:
            res = orc.map_pairs(rd["q1"], rd["o1"], rd["q2"], rd["o2"], opts=oopts, nthreads=4, want_ints=ints)
        _refs[key] = (res, ints)
    what = "k=%d L=%d %s %s%s" % (k, L, image, variant, ", single-end" if single else "")
    return (idx, rd) + _refs[key] + (what,)


def _status_ok(er, variant, what):
    """-s: bits 8 and up count the reads of the slow pass, and this data sends many there"""
    sel = variant.startswith("selAln") or variant.startswith("mimic")
    assert (er.status & 0xff if sel else er.status) == 0, (what, er.status)


def _run(root, oracle_mod, k, L, image, variant, ns=2, kernels="host", monkeypatch=None):
    """one paired call through the oracle and the emulation"""
    import emu
    idx, rd, res, ints, what = _ref(root, oracle_mod, k, L, image, variant)
    what += " ns=%d %s" % (ns, kernels)
    for name, v in KERNELS[kernels].items():
        monkeypatch.setenv(name, v)
    _, eopts = rc.opts_for(variant, oracle_mod, emu.default_opts)
    er = _emu(idx, image)[2].map(rd["q1"], rd["o1"], rd["q2"], rd["o2"], opts=eopts, ns=ns)
    _status_ok(er, variant, what)
    rc.check(res, er, what, ints=(er.int_offsets, er.ints) if ints else None)
    print("%s: %d pairs, %d hits, %r%s" % (what, rd["n"], len(res.hits), res.counters, ", %d reads on the slow pass of -s" % (er.status >> 8) if er.status >> 8 else ""))
    return res, er


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
    import emu
    idx = _index(root, 31, "dense")
    ix, orc, em = _emu(idx)
    a = rc.mixed(31, 100, extra)
    oopts, eopts = rc.opts_for(variant, oracle_mod, emu.default_opts)
    ints = oopts.selAln == 0
    res = orc.map_pairs(*a, opts=oopts, nthreads=4, want_ints=ints)
    er = em.map(*a, opts=eopts, ns=ns)
    what = "k=31 L=100 + one pair of %d, %s ns=%d" % (extra, variant, ns)
    if extra > 512 and ints:
        assert er.status == 2 << 8, (what, er.status)        # (bits 8 and up: the two reads of the long-read pass)
    else:
        _status_ok(er, variant, what)
    rc.check(res, er, what, ints=(er.int_offsets, er.ints) if ints else None)
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
    import emu
    idx, rd, res, _, what = _ref(root, oracle_mod, k, L, "dense", variant, single=True)
    q, o = pack(rc.odd_single(rd["r1"], rd["r2"]))
    er = _emu(idx)[2].map(q, o, opts=rc.opts_for(variant, oracle_mod, emu.default_opts)[1], ns=ns)
    _status_ok(er, variant, what)
    rc.check(res, er, "%s ns=%d" % (what, ns))


@pytest.mark.parametrize("k,image", [(31, "dense"), (31, "ph_compact"), (21, "dense"), (15, "dense")])
def test_what_the_pair_and_lean_kernels_leave(root, oracle_mod, k, image, capfd, monkeypatch):
    """the reads the pair and the lean kernel leave are pinned, and among the reads they KEEP there are reads whose hit list comes from one
    interval that lists a transcript more than once: their per-transcript minimum over the parked suffixes had to choose"""
    import emu
    idx, rd, res, ints, what = _ref(root, oracle_mod, k, 100, image, "default")
    monkeypatch.setenv("QM_EMU_LEAN_STATS", "2")
    capfd.readouterr()
    er = _emu(idx, image)[2].map(rd["q1"], rd["o1"], rd["q2"], rd["o2"])
    err = capfd.readouterr().err
    assert er.status == 0
    left, which = rc.emu_left(err), rc.emu_left_reads(err)
    assert len(which["pair"]) == left["pair"] and len(which["lean"]) == left["lean"]
    rep = rc.reads_with_repeated_interval(_emu(idx)[0], res)
    got = {"pair": left["pair"], "lean": left["lean"]}
    for name in ("pair", "lean"):
        kept = rep.copy()
        kept[sorted(which[name])] = False
        got[name + "_kept_repeated"] = int(kept.sum())
    print("%s: of %d reads (%d with a repeated interval) the emulation's pair / lean kernels left and kept %r" % (what, 2 * rd["n"], int(rep.sum()), got))
    assert got["pair_kept_repeated"] > 0 and got["lean_kept_repeated"] > 0, got
    assert got == EXPECT_LEFT[(k, image)], (k, image, got)


@pytest.mark.parametrize("k,L", [(31, 100), (21, 100), (15, 100), (31, 150), (31, 250)])
def test_the_data_reaches_the_repeats(root, oracle_mod, k, L):
    """repeat_cases.reach on the oracle alone: negative positions, intervals that list a transcript twice in every width the code
    distinguishes, intervals beyond maxInterval 50 and 1000; the counts are pinned"""
    idx = _index(root, k, "dense")
    ix, orc, _ = _emu(idx)
    got = rc.reach(ix, orc, oracle_mod, rc.reads_for(k, L), L, k)
    print("reach, k=%d L=%d: negative single-end %d, negative orphans %d, repeated intervals <= 64 / <= pfcap(3) / above: %d / %d / %d, intervals >= 50: %d, >= 1000: %d" % ((k, L) + got))
    rc.assert_reach(got, "k=%d L=%d" % (k, L), rc.pfcap(3, L, k))
    assert got == rc.REACH[(k, L)], got


@pytest.mark.parametrize("L", [100, 150, 250])
def test_oracle_holds_the_leftmost_positions(root, oracle_mod, L):
    """repeat_cases.truth_check on the ORACLE's hits, paired and single-end: the reference of every comparison here reports each covered
    mate on its own transcript at the leftmost place its characters occur there (and so does the emulation, which equals it)"""
    tx = rc.txome(31)
    idx, rd, res, _, what = _ref(root, oracle_mod, 31, L, "dense", "default")
    got = rc.truth_check(res.hit_offsets, res.hits, rd, tx, 31)
    print("truth_check, %s: %d eligible mates, %d checked, %d at a negative position, left out %r" % ((what,) + got))
    idx, rd, rs, _, what = _ref(root, oracle_mod, 31, L, "dense", "default", single=True)
    got = rc.truth_check(rs.hit_offsets, rs.hits, rd, tx, 31, single=True)
    print("truth_check, %s: %d eligible mates, %d checked, %d at a negative position, left out %r" % ((what,) + got))
