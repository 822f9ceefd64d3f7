"""The fragment GC bias model on the device (qm_gcb_*: rapmap_amd.GCBias) against the restatements in gcb_cases.py: window_gc over the
rank structure, classify() over the hits themselves, expect() from prefix sums.  Exact equality everywhere.  The crafted world is an
index built from the crafted transcripts (upper-case ACGT: what an index keeps of a FASTA file; lower case and N are the lane
emulation's part, test_gc_bias.py).  Run on the MI355X box: -m gpu."""
import os

import numpy as np
import pytest

import fld_cases as fc
import gcb_cases as gc
import part_cases as pc
from conftest import load_oracle
from util import pack

pytestmark = pytest.mark.gpu


def _world_of(qi):
    text, off = qi.arrays()
    w = {"text": text, "off": off, "lens": np.asarray(qi.txp_lens, dtype=np.int64)}
    for a in w.values():
        a.setflags(write=False)
    return w


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    import rapmap_amd as ra
    seqs = gc.crafted_seqs(plain_only=True)
    d = tmp_path_factory.mktemp("gcb")
    fa = str(d / "t.fa")
    with open(fa, "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b">t%d\n" % i + s + b"\n")
    idx = str(d / "idx")
    ra.build_index(fa, idx, threads=4)
    qi = ra.QuasiIndex(idx)
    mp = ra.QuasiMapper(qi, 0, debug=False)
    w = _world_of(qi)
    ref = gc.make_world(seqs)
    assert np.array_equal(w["text"][: ref["text"].size], ref["text"]) and np.array_equal(w["off"], ref["off"]) and np.array_equal(w["lens"], ref["lens"])
    yield {"world": w, "mp": mp, "qi": qi}
    mp.close(); qi.close()


def _new(mp):
    import rapmap_amd as ra
    return lambda max_len, max_blocks: ra.GCBias(mp, max_len=max_len, max_blocks=max_blocks)


def test_window_gc(crafted):
    gc.check_window_gc(crafted["world"], _new(crafted["mp"]))


@pytest.mark.parametrize("check", sorted(gc.EXPECT_CHECKS))
def test_expect(crafted, check):
    gc.EXPECT_CHECKS[check](crafted["world"], _new(crafted["mp"]))


@pytest.mark.parametrize("check", sorted(gc.OBS_CHECKS))
def test_observed(crafted, check):
    gc.OBS_CHECKS[check](crafted["world"], _new(crafted["mp"]))


def test_host_arrays_beyond_one_part(crafted):
    """(1 << 21) + 65 hits through add_hits: one more than a part of host arrays takes, so the driver uploads and sweeps twice"""
    off, h = pc.big_batch()
    h = h.copy()
    rng = np.random.default_rng(8)
    T = crafted["world"]["lens"].size
    h["tid"] = rng.integers(0, T + 1, h.size); h["pos"] = rng.integers(-5, 200, h.size); h["mate_pos"] = rng.integers(-5, 200, h.size)
    h["frag_len"] = rng.integers(0, 140, h.size)
    f = _new(crafted["mp"])(100, 0)
    try:
        f.add_hits(off, h)
        c, s = f.counts(), f.stat()
    finally:
        f.close()
    eo, es = gc.classify(crafted["world"], off, h, 100)
    gc.assert_same(c, s, eo, es, "2 097 217 hits")
    assert s["folds"] == 2 and es["used"] > 1000 and es["overhang"] > 1000 and es["out_of_range"] > 1000


def test_times_and_errors(crafted):
    import rapmap_amd as ra
    mp = crafted["mp"]
    for bad, code in ((0, "-1"), (-5, "-1"), (1024, "-4")):         # QM_E_ARG, QM_E_ARG, QM_E_UNSUPPORTED
        with pytest.raises(ra.QmError, match=code):
            ra.GCBias(mp, max_len=bad)
    fresh = ra.QuasiMapper(crafted["qi"], 0)
    g = ra.GCBias(fresh)
    with pytest.raises(ra.QmError, match="-7"):                     # QM_E_STATE: no result yet
        g.add(fresh)
    with pytest.raises(ra.QmError, match="-1"):
        g.add_hits([0, 2, 1], np.zeros(2, dtype=ra.HIT_DTYPE))      # offsets that decrease
    assert all(v == 0 for k, v in g.stat().items() if k not in ("max_len", "rank_build_us"))
    off, h = gc.random_batch(crafted["world"], 500, 1000, seed=1)
    g.add_hits(off, h)
    g.expect(gc.histograms(crafted["world"], 1000)["sparse"], crafted["world"]["lens"].size)
    s = g.stat()
    assert s["last_fold_us"] > 0 and s["last_expect_us"] > 0 and s["folds"] == 1
    g.close(); fresh.close()


@pytest.fixture(scope="module")
def small(synth_small):
    import rapmap_amd as ra
    qi = ra.QuasiIndex(synth_small["idx"])
    mp = ra.QuasiMapper(qi, 0, debug=False)
    q1, o1 = pack(synth_small["reads1"]); q2, o2 = pack(synth_small["reads2"])
    yield {"qi": qi, "mp": mp, "q1": q1, "o1": o1, "q2": q2, "o2": o2, "world": _world_of(qi)}
    mp.close()


def test_synth_small_pairs(small, synth_small, oracle_mod):
    """the mapper's own result swept where it lies, against the oracle's hits; then the expected matrix of that run's fragment lengths
    and the effective lengths from both"""
    import rapmap_amd as ra
    mp, w = small["mp"], small["world"]
    ix, orc = load_oracle(synth_small["idx"])
    res = orc.map_pairs(small["q1"], small["o1"], small["q2"], small["o2"], nthreads=4)
    eo, es = gc.classify(w, res.hit_offsets, res.hits, 1000)
    mp.map_pairs(small["q1"], small["o1"], small["q2"], small["o2"])
    g = ra.GCBias(mp)
    g.add(mp)
    gc.assert_same(g.counts(), g.stat(), eo, es, "synth_small: the oracle's hits")
    assert es["units"] == 4234 and es["used"] >= 500 and g.stat()["folds"] == 1 and g.stat()["last_fold_us"] > 0
    counts, _ = fc.classify(res.hit_offsets, res.hits, 1000)
    T = w["lens"].size
    H = g.expect(counts, T)
    assert np.array_equal(H, gc.expect(w, counts))
    gc.assert_identity(w, counts, H, "synth_small")
    alpha = np.ones(T, dtype=np.float64)
    got = ra.gc_eff_lens_from_counts(counts, w["lens"], H, alpha, g.counts())
    exp = gc.eff_lens(counts, w["lens"], H, alpha, eo)
    for a, b in zip(got, exp):
        assert a.tobytes() == b.tobytes()
    g.close()


def test_synth_small_single_end(small, synth_small, oracle_mod):
    import rapmap_amd as ra
    mp = small["mp"]
    ix, orc = load_oracle(synth_small["idx"])
    rs = orc.map_single(small["q1"], small["o1"], nthreads=4)
    eo, es = gc.classify(small["world"], rs.hit_offsets, rs.hits, 1000)
    mp.map_reads(small["q1"], small["o1"])
    g = ra.GCBias(mp)
    g.add(mp)
    gc.assert_same(g.counts(), g.stat(), eo, es, "single-end: the oracle's hits")
    assert es["used"] == 0 and es["not_paired"] + es["unmapped"] + es["multi"] == es["units"] and es["not_paired"] > 500
    g.close()


def test_another_index_is_refused(small, crafted):
    import rapmap_amd as ra
    small["mp"].map_pairs(small["q1"], small["o1"], small["q2"], small["o2"])
    g = ra.GCBias(crafted["mp"])
    with pytest.raises(ra.QmError, match="-1"):                     # QM_E_ARG: the object's rank structure is another index's
        g.add(small["mp"])
    g.close()


# ---- the stream and the CLI on synth_small

@pytest.fixture(scope="module")
def oracle_small(small, synth_small, oracle_mod):
    """the oracle's hits of synth_small restated: fragment lengths and observed GC counts (shared; never changed)"""
    ix, orc = load_oracle(synth_small["idx"])
    res = orc.map_pairs(small["q1"], small["o1"], small["q2"], small["o2"], nthreads=4)
    counts, _ = fc.classify(res.hit_offsets, res.hits, 1000)
    obs, st = gc.classify(small["world"], res.hit_offsets, res.hits, 1000)
    return {"counts": counts, "obs": obs, "stats": st}


@pytest.fixture(scope="module")
def small_fastq(synth_small, tmp_path_factory):
    d = tmp_path_factory.mktemp("gcb_fq")
    f1, f2 = str(d / "r1.fastq"), str(d / "r2.fastq")
    for fn, nms, rds in ((f1, synth_small["names1"], synth_small["reads1"]), (f2, synth_small["names2"], synth_small["reads2"])):
        with open(fn, "wb") as fh:
            for nm, r in zip(nms, rds):
                fh.write(b"@" + nm.encode() + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
    return f1, f2


def test_stream(small, oracle_small, small_fastq):
    import rapmap_amd as ra
    f1, f2 = small_fastq
    plain = ra.MappedStream(small["qi"], f1, f2, batch_units=512, threads=3, names=False, eq_classes=True, hits=False)
    for b in plain:
        pass
    table = plain.eq_classes()
    with pytest.raises(ra.QmError, match="-7"):                   # QM_E_STATE: opened without gc_bias
        plain.gc_bias()
    assert plain.stats()["gcb_sweep_s"] == 0
    plain.close()
    for classes in (False, True):
        st = ra.MappedStream(small["qi"], f1, f2, batch_units=512, threads=3, names=False, eq_classes=classes, hits=not classes, frag_len_dist=classes, gc_bias=True)
        with pytest.raises(ra.QmError, match="-7"):               # QM_E_STATE: the input has not ended
            st.gc_bias()
        nb = 0; per_batch = np.zeros(gc.NB, dtype=np.uint64)
        for b in st:
            nb += 1
            if not classes:
                per_batch += gc.classify(small["world"], b.hit_offsets, b.hits, 1000)[0]
        obs, stats = st.gc_bias()
        assert nb == 9 and st.stats()["gcb_sweep_s"] > 0
        gc.assert_same(obs, stats, oracle_small["obs"], oracle_small["stats"], "stream, eq_classes=%s" % classes)
        if classes:
            for x, y in zip(st.eq_classes(), table):
                assert x.tobytes() == y.tobytes()                 # the same class table with and without the sweep
            assert np.array_equal(st.frag_len_dist()[0], oracle_small["counts"])
        else:
            assert np.array_equal(per_batch, obs)                 # the sum over its batches
        st.close()


def test_stream_with_every_tally(small, small_fastq):
    """one stream with all four kinds of per-context tally on gives, bit for bit, what the streams with one kind each give: the class table
    of a stream with the classes and the library type alone, and the histogram, the GC counts and the library-type tallies of the
    single-flag streams"""
    import rapmap_amd as ra
    f1, f2 = small_fastq

    def run(**flags):
        st = ra.MappedStream(small["qi"], f1, f2, batch_units=512, threads=3, names=False, **flags)
        nb = sum(1 for _ in st)
        assert nb == 9
        return st

    st = run(eq_classes=True, lib_type="IU")
    table, lib_with_classes = st.eq_classes(), st.lib_counts()
    st.close()
    st = run(frag_len_dist=True)
    fld = st.frag_len_dist()
    st.close()
    st = run(gc_bias=True)
    gcb = st.gc_bias()
    st.close()
    st = run(lib_type="IU")
    lib = st.lib_counts()
    st.close()
    assert np.array_equal(lib, lib_with_classes)                  # (tallied the same with and without the fold behind it)

    st = run(eq_classes=True, hits=False, frag_len_dist=True, gc_bias=True, lib_type="IU")
    for x, y in zip(st.eq_classes(), table):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    counts, stats = st.frag_len_dist()
    assert counts.tobytes() == fld[0].tobytes() and stats == fld[1]
    obs, gstats = st.gc_bias()
    assert obs.tobytes() == gcb[0].tobytes() and gstats == gcb[1]
    assert st.lib_counts().tobytes() == lib.tobytes()
    s = st.stats()
    assert s["fold_s"] > 0 and s["fld_fold_s"] > 0 and s["gcb_sweep_s"] > 0
    st.close()


def _cli(args):
    import subprocess
    import sys
    from conftest import ROOT
    return subprocess.run([sys.executable, "-m", "rapmap_amd", "quasimap"] + args, cwd=ROOT, capture_output=True, text=True)


def _small_args(synth_small):
    from conftest import GOLD
    sd = os.path.join(GOLD, "synth_small")
    return ["-i", synth_small["idx"], "-1", os.path.join(sd, "reads_1.fastq.gz"), "-2", os.path.join(sd, "reads_2.fastq.gz"), "-t", "4", "-n"]


def _table(small):
    """a class table filled the way the CLI fills its own (a table of the default size, the sorted classes in one add_labels: equal
    input gives equal slots, hence the same order of every sum)"""
    import rapmap_amd as ra
    mp = small["mp"]
    mp.map_pairs(small["q1"], small["o1"], small["q2"], small["o2"])
    src = ra.EqClasses(mp); src.add(mp)
    t = ra.EqClasses(mp); t.add_labels(*src.fetch())
    src.close()
    return t


def test_cli_quant_gc_bias(small, synth_small, oracle_small, tmp_path):
    import rapmap_amd as ra
    qf = str(tmp_path / "q.sf")
    r = _cli(_small_args(synth_small) + ["--quant", qf, "--quantFLD", "--quantGCBias"])
    assert r.returncode == 0, r.stderr
    assert "fragment GC: units 4234, used %d" % oracle_small["stats"]["used"] in r.stderr and "overhang %d" % oracle_small["stats"]["overhang"] in r.stderr
    names, lens, eff, tpm, reads = ra.read_quant(qf)
    w, counts, obs = small["world"], oracle_small["counts"], oracle_small["obs"]
    T = small["qi"].n_txps
    # by hand: the first estimate on the fragment-length effective lengths, the restated matrix, the restated arithmetic, a second
    # estimate on its effective lengths started from the first
    t = _table(small)
    q1 = ra.Quant(t, T, fc.eff_lens(counts, lens)); q1.run(); first = q1.fetch(); q1.close()
    H = gc.expect(w, counts)
    exp_eff, exp_exp, exp_ratio = gc.eff_lens(counts, lens, H, first, obs)
    assert eff.tobytes() == exp_eff.tobytes()                     # (write_quant prints repr, read_quant's float() gives every bit back)
    q2 = ra.Quant(t, T, exp_eff); q2.set_start(first); q2.run(); second = q2.fetch(); q2.close(); t.close()
    assert reads.tobytes() == second.tobytes()
    assert (exp_ratio != 1.0).any() and not np.array_equal(first, second)
    o_, e_, r_ = ra.read_gc_bias(qf + ".gcBias.txt")
    assert np.array_equal(o_, obs) and e_.tobytes() == exp_exp.tobytes() and r_.tobytes() == exp_ratio.tobytes()
    assert os.path.exists(qf + ".flenDist.txt")


def test_cli_without_the_flag_is_unchanged(small, synth_small, oracle_small, tmp_path):
    """no --quantGCBias: quant.sf is what --quantFLD wrote before, and no gcBias file is written"""
    import rapmap_amd as ra
    qf, mine = str(tmp_path / "q.sf"), str(tmp_path / "mine.sf")
    r = _cli(_small_args(synth_small) + ["--quant", qf, "--quantFLD"])
    assert r.returncode == 0, r.stderr
    assert "fragment GC" not in r.stderr and not os.path.exists(qf + ".gcBias.txt") and "gcb_sweep_s 0.000" in r.stderr
    lens = np.asarray(small["qi"].txp_lens, dtype=np.int64)
    eff = fc.eff_lens(oracle_small["counts"], lens)
    t = _table(small)
    q = ra.Quant(t, small["qi"].n_txps, eff); q.run(); alpha = q.fetch(); q.close(); t.close()
    ra.write_quant(mine, small["qi"].txp_names, lens, eff, alpha)
    assert open(qf, "rb").read() == open(mine, "rb").read()
