"""Reads that hang over a transcript end and transcripts shorter than a read (ends_cases.py), through the device mapper's source under the
lane emulation (tests/emu), against the oracle: bit-exact hits, offsets, counters and SA-interval lists, and `status == 0` (the
emulation's own cross-checks of the pair, lean and packed kernels against the general one).  The same data runs on the HIP path in
test_txp_ends_gpu.py (-m gpu).

The branches this reaches: negative positions in sel_side_score (qm_sel.inl: invalidStart / invalidEnd, `dropped` under alignment
policies 1 and 2, targets shorter than the query), the clamps of the pair kernel's merge (qm_lean.inl), the signed sort key and
`fragEnd - fragStart` with negative starts (qm_mapper.inl), and extension tables whose entries stop at a `$` or the end of the text.
Every test that maps asserts ends_cases.reach()'s minimums on the oracle's own result and prints the counts."""
import numpy as np
import pytest

import ends_cases as ec
import fld_cases as fc
from conftest import load_oracle
from util import pack

_emus, _refs = {}, {}


def _emu(idx):
    """(index as the oracle reads it, oracle, emulation) of an index, kept for the process"""
    import emu
    if idx not in _emus:
        ix, orc = load_oracle(idx)
        _emus[idx] = (ix, orc, emu.Emu(ix))
    return _emus[idx]


@pytest.fixture(scope="module")
def root(tmp_path_factory, lib_built, oracle_mod):
    return tmp_path_factory.mktemp("txp_ends")


def _ref(root, oracle_mod, k, L, image, variant, single=False):
    """the oracle's result of one configuration, computed once and shared (never changed), with its reach asserted.
    -> (idx, read set, result, keeps intervals?)"""
    key = (k, L, image, variant, single)
    idx = ec.index_for(root, k, image)
    rd = ec.reads_for(k, L)
    if key not in _refs:
        import emu
        ix, orc, em = _emu(idx)
        oopts, _ = ec.opts_for(variant, oracle_mod, emu.default_opts)
        ints = not single and oopts.selAln == 0
        what = "k=%d L=%d %s %s%s" % (k, L, image, variant, ", single-end" if single else "")
        if single:
            q, o = pack(ec.odd_single(rd["r1"], rd["r2"]))
            assert (len(o) - 1) % 2 == 1
            res = orc.map_single(q, o, opts=oopts, nthreads=4)
            n = len(o) - 1
        else:
            res = orc.map_pairs(rd["q1"], rd["o1"], rd["q2"], rd["o2"], opts=oopts, nthreads=4, want_ints=ints)
            n = rd["n"]
        ec.report("oracle, " + what, n, res, ec.assert_reach(res, rd["lens"], L, variant, what))
        _refs[key] = (res, ints, what)
    return (idx, rd) + _refs[key]


def _run(root, oracle_mod, k, L, image, variant, ns=2):
    """one paired call through the oracle and the emulation"""
    import emu
    idx, rd, res, ints, what = _ref(root, oracle_mod, k, L, image, variant)
    _, eopts = ec.opts_for(variant, oracle_mod, emu.default_opts)
    er = _emu(idx)[2].map(rd["q1"], rd["o1"], rd["q2"], rd["o2"], opts=eopts, ns=ns)
    assert er.status == 0, (what, er.status)
    ec.check(res, er, what, ints=(er.int_offsets, er.ints) if ints else None)
    return res, er


@pytest.mark.parametrize("variant", sorted(ec.OPTION_SETS))
def test_pairs_k31(root, oracle_mod, variant):
    """2 x 100 at k = 31, every option set"""
    _run(root, oracle_mod, 31, 100, "dense", variant)


@pytest.mark.parametrize("variant", ec.FEW)
@pytest.mark.parametrize("k,L,image,ns", [(21, 100, "dense", 2), (21, 100, "ph", 2), (31, 64, "dense", 2), (31, 150, "dense", 3), (15, 250, "dense", 4)])
def test_pairs_other_shapes(root, oracle_mod, k, L, image, ns, variant):
    """other k, a -p index, reads of one slot and of three and four (the wide editions)"""
    _run(root, oracle_mod, k, L, image, variant, ns=ns)


@pytest.mark.parametrize("variant", ["default", "selAln"])
@pytest.mark.parametrize("k,L,ns", [(31, 100, 2), (21, 150, 3)])
def test_single_end(root, oracle_mod, k, L, ns, variant):
    """single-end, an odd count"""
    import emu
    idx, rd, res, _, what = _ref(root, oracle_mod, k, L, "dense", variant, single=True)
    q, o = pack(ec.odd_single(rd["r1"], rd["r2"]))
    er = _emu(idx)[2].map(q, o, opts=ec.opts_for(variant, oracle_mod, emu.default_opts)[1], ns=ns)
    assert er.status == 0, (what, er.status)
    ec.check(res, er, what)


def test_oracle_holds_the_true_positions(root, oracle_mod):
    """ends_cases.truth_check on the ORACLE's hits, paired and single-end: the reference of every comparison here finds each covered mate
    on its own transcript at the position it was cut from, negative ones included (and so does the emulation, which equals it)"""
    idx, rd, res, _, what = _ref(root, oracle_mod, 31, 100, "dense", "default")
    got = ec.truth_check(res.hit_offsets, res.hits, ec.covered(rd["truth"], 31))
    print("truth_check, %s: %d mates, %d with a negative position" % ((what,) + got))
    idx, rd, rs, _, what = _ref(root, oracle_mod, 31, 100, "dense", "default", single=True)
    got = ec.truth_check(rs.hit_offsets, rs.hits, None, single=ec.covered_single(rd["truth"], 31))
    print("truth_check, %s: %d mates, %d with a negative position" % ((what,) + got))


@pytest.mark.parametrize("variant", ["default", "selAln"])
def test_sam_writer(root, oracle_mod, variant):
    """the native SAM writer (host code, qm_io.cpp: clipping after adjustOverhang) on hits that hang over both ends and lie on transcripts
    shorter than the read: line for line what samfmt formats from the same hits, paired and single-end"""
    import rapmap_amd as ra
    import samfmt as sam
    idx, rd, res, _, what = _ref(root, oracle_mod, 31, 100, "dense", variant)
    ix = _emu(idx)[0]
    qi = ra.QuasiIndex(idx)
    try:
        n = rd["n"]
        nm1 = ["p%d/1" % i for i in range(n)]; nm2 = ["p%d/2" % i for i in range(n)]
        b = ra.ReadBatch(); b.n = n
        b.seq1, b.off1, b.seq2, b.off2 = rd["q1"], rd["o1"], rd["q2"], rd["o2"]
        b.names1, b.name_off1 = pack([x.encode() for x in nm1]); b.names2, b.name_off2 = pack([x.encode() for x in nm2])
        got = ra.sam_records_text(qi, b, res.hit_offsets, res.hits, threads=3).decode().splitlines(True)
        want = "".join(sam.format_pair(nm1[i], rd["r1"][i], nm2[i], rd["r2"][i], res.hits[res.hit_offsets[i]:res.hit_offsets[i + 1]], ix.names, ix.txpLens)
                       for i in range(n)).splitlines(True)
        assert got == want, what
        assert sum("S" in l.split("\t")[5] for l in want) > 500, "hardly a record is clipped"
        _, _, rs, _, what = _ref(root, oracle_mod, 31, 100, "dense", variant, single=True)
        one = ec.odd_single(rd["r1"], rd["r2"])
        sb = ra.ReadBatch(); sb.n = len(one)
        sb.seq1, sb.off1 = pack(one)
        names = ["s%d" % i for i in range(len(one))]
        sb.names1, sb.name_off1 = pack([x.encode() for x in names])
        got = ra.sam_records_text(qi, sb, rs.hit_offsets, rs.hits, threads=2).decode().splitlines(True)
        want = "".join(sam.format_single(names[i], one[i], rs.hits[rs.hit_offsets[i]:rs.hit_offsets[i + 1]], ix.names, ix.txpLens) for i in range(sb.n)).splitlines(True)
        assert got == want, what
    finally:
        qi.close()


def test_fragment_lengths(root, oracle_mod):
    """the fragment-length sweep under its lane emulation over the oracle's hits of this data (fragment lengths of pairs with negative
    starts), and the effective lengths from that histogram for every transcript, the 1-, 5- and (k - 1)-character ones included: the
    library's host arithmetic against fld_cases' restatement, bit for bit"""
    import emu_fld
    import rapmap_amd as ra
    idx, rd, res, _, what = _ref(root, oracle_mod, 31, 100, "dense", "default")
    counts, st = fc.check_against_restatement(emu_fld.EmuFld, res.hit_offsets, res.hits, max_blocks=3, what=what)
    print("fragment lengths, %s: %r" % (what, st))
    assert st["units"] == rd["n"] and st["used"] >= 100, st
    lens = rd["lens"]
    assert lens.min() == 1 and (lens == 5).any() and (lens == 30).any()
    assert ra.eff_lens_from_counts(counts, lens).tobytes() == fc.eff_lens(counts, lens).tobytes()
