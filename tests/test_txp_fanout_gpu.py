"""Families of T transcripts around a shared core (fanout_cases.py) on the HIP path (libqmap_mi355.so through its C ABI), against the
oracle: bit-exact hits, offsets and counters from the kernels the headline is quoted on -- qm_lean_kernel, whose hits-to-mappings pass
(lean_h2m, qm_lean.inl) works in 8 x 8 tiles over the wavefront for 3 .. 32 suffixes, and the pair kernel -- and from the lean kernel's
edition for the compact -p image.  Each kernel leaves exactly the reads the lane emulation of the same source leaves
(test_txp_fanout.py runs the same data there)."""
import pytest

import fanout_cases as fc
import kmer_cases as kc
import mapping_harness as mh
import rapmap_amd as ra

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def root(tmp_path_factory, lib_built, oracle_mod):
    return tmp_path_factory.mktemp("txp_fanout_gpu")


def emu_left(root, oracle_mod, image, capfd, monkeypatch):
    """the reads the emulation's pair and lean kernels leave under default options"""
    r = mh.ref(fc, root, oracle_mod, 31, 100, image, "default")
    monkeypatch.setenv("QM_EMU_LEAN_STATS", "1")
    capfd.readouterr()
    er = mh.emu_of(r.idx, image)[2].map(*r.a)
    left = kc.emu_left(capfd.readouterr().err)
    assert er.status == 0, er.status
    mh.check(r.res, er, "emulation, " + r.what)
    return left


@pytest.mark.parametrize("kernel", mh.HEADLINE_KERNELS)
def test_headline_kernels(root, oracle_mod, kernel, capfd, monkeypatch):
    left = emu_left(root, oracle_mod, "dense", capfd, monkeypatch)
    idx = fc.index_for(root, 31, "dense")
    with mh.headline(idx, kernel) as (qi, mp):
        for variant in fc.VARIANTS:
            r = mh.ref(fc, root, oracle_mod, 31, 100, "dense", variant)
            tm = mh.Timer("%s kernel, %s" % (kernel, r.what))
            gr = mp.map_pairs(*r.a, opts=mh.lib_opts(variant, oracle_mod))
            mh.check(r.res, gr, tm.what)
            tm.done(1)
            assert mp.stat(ra.QM_STAT_LEAN_READS) == 2 * r.n, "the %s kernel did not run" % kernel
            if variant == "default":
                deferred = mh.check_headline(mp, kernel, r.n)
                assert deferred == left[kernel], (kernel, deferred, left)


def test_lean_kernel_compact_ph(root, oracle_mod, capfd, monkeypatch):
    """the compact -p image, where the host launches qm_lean_kernel's PH edition"""
    left = emu_left(root, oracle_mod, "ph_compact", capfd, monkeypatch)
    mh.lean_kernel_compact_ph(fc, root, oracle_mod, 31, lean_sets=("default",), expect_left=left["lean"], timed=True)
