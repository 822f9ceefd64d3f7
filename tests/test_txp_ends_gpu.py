"""Reads that hang over a transcript end and transcripts shorter than a read (ends_cases.py) on the HIP path (libqmap_mi355.so through its
C ABI), against the oracle: bit-exact hits, offsets, counters and -- where the general kernel keeps them -- SA-interval lists.  The lane
emulation of the same source runs the same data in test_txp_ends.py; what only this module sees is the host's tables, the packed table
builders on a text this small (a `$` right behind many k-mers, the last k-mer ending the text), the real wave execution and the pair
kernel's merge in LDS.

Every index is built once per module, every oracle result once (shared, never changed); every test that maps asserts
ends_cases.reach()'s minimums on the oracle's own result and prints the counts."""
import pytest

import ends_cases as ec
import mapping_harness as mh
import rapmap_amd as ra
from util import pack

pytestmark = pytest.mark.gpu

HEADLINE_SETS = ("default", "fuzzy", "noDovetail", "noOrphans", "selAln")


@pytest.fixture(scope="module")
def root(tmp_path_factory, lib_built, oracle_mod):
    return tmp_path_factory.mktemp("txp_ends_gpu")


def test_general_kernel_k31(root, oracle_mod):
    """every option set at k = 31, 2 x 100, with the interval lists where -s is off"""
    mh.general_kernel(ec, root, oracle_mod, 31, 100, "dense", sorted(ec.OPTION_SETS))


@pytest.mark.parametrize("k,L,image,ph_compact", [(21, 100, "dense", False), (21, 100, "ph", False), (21, 100, "ph", True), (31, 64, "dense", False),
                                                  (31, 150, "dense", False), (15, 250, "dense", False)])
def test_general_kernel_other_shapes(root, oracle_mod, k, L, image, ph_compact):
    mh.general_kernel(ec, root, oracle_mod, k, L, image, ec.FEW, ph_compact=ph_compact)


@pytest.mark.parametrize("kernel", ["pair", "lean"])
@pytest.mark.parametrize("k", [31, 21])
def test_headline_kernels(root, oracle_mod, k, kernel):
    """the pair kernel (its own merge: positions clamped at 0 before the dovetail test, the orphan left of the transcript start under
    --noDovetail) and qm_lean_kernel: both ran, and the pair kernel merged some pairs of this data itself"""
    with mh.headline(ec.index_for(root, k, "dense"), kernel) as (qi, mp):
        for variant in HEADLINE_SETS:
            r = mh.ref(ec, root, oracle_mod, k, 100, "dense", variant)
            gr = mp.map_pairs(*r.a, opts=mh.lib_opts(variant, oracle_mod))
            mh.check(r.res, gr, "%s kernel, %s" % (kernel, r.what))
            assert mp.stat(ra.QM_STAT_LEAN_READS) == 2 * r.n, "the %s kernel did not run" % kernel
            if kernel == "pair" and variant == "default":
                merged = mp.stat(ra.QM_STAT_PAIRS_MERGED)
                print("pair kernel, %s: merged %d of %d pairs itself" % (r.what, merged, r.n))
                assert merged > 0


@pytest.mark.parametrize("k", [31, 21])
def test_lean_kernel_compact_ph(root, oracle_mod, k):
    """the compact -p image, where the host launches qm_lean_kernel's PH edition"""
    mh.lean_kernel_compact_ph(ec, root, oracle_mod, k, lean_sets=("default", "selAln"))


@pytest.mark.parametrize("k,L", [(31, 150), (17, 250)])
def test_wide_lean_kernel(root, oracle_mod, k, L):
    """reads of 150 and 250 characters: the wide lean kernel (one read per wavefront) on SaExt2 entries that stop at a `$` after none or a
    few characters; paired and single-end"""
    mh.wide_lean_kernel(ec, root, oracle_mod, k, L)


@pytest.mark.parametrize("debug", [True, False])
def test_single_end(root, oracle_mod, debug):
    """single-end, an odd count, through the general kernel and the lean kernel"""
    mh.single_end(ec, root, oracle_mod, debug, lean_sets=("default", "selAln"))


def test_packed_reads_and_stage_view(root, oracle_mod):
    """the reads sent 2-bit packed (map_pairs_packed) give the fused result; the stage entry points (map_pairs_stages, with and without
    intervals, reads as characters and packed) give it unit by unit but for the units whose excess orphans only the caller drops"""
    mh.packed_reads_and_stage_view(ec, root, oracle_mod)


@pytest.mark.parametrize("k", [31, 17])
def test_table_builders(root, oracle_mod, k, monkeypatch):
    """QM_TABLE_CHECK=1 holds every entry of SaExt / SaExt2 / sanext as the packed builders made it against the byte-per-character builders
    and fails the build on a difference -- on a text where a `$` follows many k-mers at once and the last k-mer ends the text: one -s call
    (sanext), one with 150-character reads (SaExt2), and one with 100-character reads on a fresh mapper (SaExt alone)"""
    monkeypatch.setenv("QM_TABLE_CHECK", "1")
    mh.table_builders(ec, root, oracle_mod, k)


@pytest.mark.parametrize("kernel", ["general", "pair"])
def test_true_positions(root, oracle_mod, kernel):
    """ends_cases.truth_check on the DEVICE's hits: no oracle, no suffix array"""
    r = mh.ref(ec, root, oracle_mod, 31, 100, "dense", "default")
    rd = r.rd
    with mh.gpu_mapper(r.idx, debug=kernel == "general") as (qi, mp):
        gr = mp.map_pairs(*r.a)
        assert mp.stat(ra.QM_STAT_LEAN_READS) == (-1 if kernel == "general" else 2 * rd["n"])
        got = ec.truth_check(gr.hit_offsets, gr.hits, ec.covered(rd["truth"], 31))
        print("truth_check, %s kernel, %s: %d mates, %d with a negative position" % ((kernel, r.what) + got))
        q, o = pack(mh.odd_single(rd["r1"], rd["r2"]))
        gs = mp.map_reads(q, o)
        ec.truth_check(gs.hit_offsets, gs.hits, None, single=ec.covered_single(rd["truth"], 31))


def test_fragment_lengths(root, oracle_mod):
    """the device's histogram over the default mapping equals fld_cases' restatement over the oracle's hits; the effective lengths from it
    equal the restatement's for every transcript, the 1-, 5- and (k - 1)-character ones included"""
    lens = mh.fragment_lengths(ec, root, oracle_mod).rd["lens"]
    assert lens.min() == 1 and (lens == 5).any() and (lens == 30).any()
