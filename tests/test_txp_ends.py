"""Reads that hang over a transcript end and transcripts shorter than a read (ends_cases.py), through the device mapper's source under the
lane emulation (tests/emu), against the oracle: bit-exact hits, offsets, counters and SA-interval lists, and `status == 0` (the
emulation's own cross-checks of the pair, lean and packed kernels against the general one).  The same data runs on the HIP path in
test_txp_ends_gpu.py (-m gpu).

The branches this reaches: negative positions in sel_side_score (qm_sel.inl: invalidStart / invalidEnd, `dropped` under alignment
policies 1 and 2, targets shorter than the query), the clamps of the pair kernel's merge (qm_lean.inl), the signed sort key and
`fragEnd - fragStart` with negative starts (qm_mapper.inl), and extension tables whose entries stop at a `$` or the end of the text.
Every test that maps asserts ends_cases.reach()'s minimums on the oracle's own result and prints the counts."""
import pytest

import ends_cases as ec
import fld_cases as fc
import mapping_harness as mh
from util import pack


@pytest.fixture(scope="module")
def root(tmp_path_factory, lib_built, oracle_mod):
    return tmp_path_factory.mktemp("txp_ends")


@pytest.mark.parametrize("variant", sorted(ec.OPTION_SETS))
def test_pairs_k31(root, oracle_mod, variant):
    """2 x 100 at k = 31, every option set"""
    mh.emu_pairs(ec, root, oracle_mod, 31, 100, "dense", variant)


@pytest.mark.parametrize("variant", ec.FEW)
@pytest.mark.parametrize("k,L,image,ns", [(21, 100, "dense", 2), (21, 100, "ph", 2), (31, 64, "dense", 2), (31, 150, "dense", 3), (15, 250, "dense", 4)])
def test_pairs_other_shapes(root, oracle_mod, k, L, image, ns, variant):
    """other k, a -p index, reads of one slot and of three and four (the wide editions)"""
    mh.emu_pairs(ec, root, oracle_mod, k, L, image, variant, ns=ns, flat_ph=False)       # (the -p index through the emulated BooPHF levels)


@pytest.mark.parametrize("variant", ["default", "selAln"])
@pytest.mark.parametrize("k,L,ns", [(31, 100, 2), (21, 150, 3)])
def test_single_end(root, oracle_mod, k, L, ns, variant):
    """single-end, an odd count"""
    mh.emu_single_end(ec, root, oracle_mod, k, L, variant, ns)


def test_oracle_holds_the_true_positions(root, oracle_mod):
    """ends_cases.truth_check on the ORACLE's hits, paired and single-end: the reference of every comparison here finds each covered mate
    on its own transcript at the position it was cut from, negative ones included (and so does the emulation, which equals it)"""
    r = mh.emu_ref(ec, root, oracle_mod, 31, 100, "dense", "default")
    got = ec.truth_check(r.res.hit_offsets, r.res.hits, ec.covered(r.rd["truth"], 31))
    print("truth_check, %s: %d mates, %d with a negative position" % ((r.what,) + got))
    r = mh.emu_ref(ec, root, oracle_mod, 31, 100, "dense", "default", single=True)
    got = ec.truth_check(r.res.hit_offsets, r.res.hits, None, single=ec.covered_single(r.rd["truth"], 31))
    print("truth_check, %s: %d mates, %d with a negative position" % ((r.what,) + got))


@pytest.mark.parametrize("variant", ["default", "selAln"])
def test_sam_writer(root, oracle_mod, variant):
    """the native SAM writer (host code, qm_io.cpp: clipping after adjustOverhang) on hits that hang over both ends and lie on transcripts
    shorter than the read: line for line what samfmt formats from the same hits, paired and single-end"""
    import rapmap_amd as ra
    import samfmt as sam
    r = mh.emu_ref(ec, root, oracle_mod, 31, 100, "dense", variant)
    idx, rd, res, what = r.idx, r.rd, r.res, r.what
    ix = mh.oracle_of(idx)[0]
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
        r = mh.emu_ref(ec, root, oracle_mod, 31, 100, "dense", variant, single=True)
        rs, what = r.res, r.what
        one = mh.odd_single(rd["r1"], rd["r2"])
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
    r = mh.emu_ref(ec, root, oracle_mod, 31, 100, "dense", "default")
    rd, res, what = r.rd, r.res, r.what
    counts, st = fc.check_against_restatement(emu_fld.EmuFld, res.hit_offsets, res.hits, max_blocks=3, what=what)
    print("fragment lengths, %s: %r" % (what, st))
    assert st["units"] == rd["n"] and st["used"] >= 100, st
    lens = rd["lens"]
    assert lens.min() == 1 and (lens == 5).any() and (lens == 30).any()
    assert ra.eff_lens_from_counts(counts, lens).tobytes() == fc.eff_lens(counts, lens).tobytes()
