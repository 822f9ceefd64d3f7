"""The positional bias model on the device (qm_psb_*: rapmap_amd.PosBias) against the restatements in psb_cases.py: classes and bins,
classify() over the hits themselves, expect() by a term per position in Python integers, eff_lens() with every float sum spelled out.
Exact equality everywhere, floats bit for bit.  The crafted world is an index built from the crafted transcripts.  Run on the MI355X
box: -m gpu."""
import os

import numpy as np
import pytest

import fld_cases as fc
import gcb_cases as gc
import part_cases as pc
import psb_cases as ps
import sqb_cases as sq
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
    seqs = ps.crafted_seqs()
    d = tmp_path_factory.mktemp("psb")
    fa = str(d / "t.fa")
    ps.write_fasta(fa, seqs)
    idx = str(d / "idx")
    ra.build_index(fa, idx, threads=4)
    qi = ra.QuasiIndex(idx)
    mp = ra.QuasiMapper(qi, 0, debug=False)
    w = _world_of(qi)
    ref = gc.make_world(seqs)
    assert np.array_equal(w["off"], ref["off"]) and np.array_equal(w["lens"], ref["lens"]) and [int(x) for x in w["lens"]] == list(ps.LENS)
    yield {"world": w, "mp": mp, "qi": qi}
    mp.close(); qi.close()


def _new(mp):
    import rapmap_amd as ra
    return lambda max_len, max_blocks: ra.PosBias(mp, max_len=max_len, max_blocks=max_blocks)


def test_positions(crafted):
    ps.check_positions(crafted["world"], _new(crafted["mp"]))


@pytest.mark.parametrize("check", sorted(ps.OBS_CHECKS))
def test_observed(crafted, check):
    ps.OBS_CHECKS[check](crafted["world"], _new(crafted["mp"]))


@pytest.mark.parametrize("check", sorted(ps.EXPECT_CHECKS))
def test_expect(crafted, check):
    ps.EXPECT_CHECKS[check](crafted["world"], _new(crafted["mp"]))


@pytest.mark.parametrize("check", sorted(ps.EFF_CHECKS))
def test_eff_lens(crafted, check):
    if check == "ratio_one":
        import rapmap_amd as ra
        ps.check_eff_ratio_one(crafted["world"], _new(crafted["mp"]), ra.eff_lens_from_counts)
    else:
        ps.EFF_CHECKS[check](crafted["world"], _new(crafted["mp"]))


def test_eff_lens_device_is_the_emulation(crafted):
    """(c) once more, three ways: device = lane emulation = restatement, bit for bit"""
    import emu_psb
    w = crafted["world"]; T = w["lens"].size
    c = ps.eff_histograms()["sparse"]; R = ps.random_ratios(97)
    d = _new(crafted["mp"])(1000, 0); e = emu_psb.EmuPsb(w["off"], w["lens"], 1000, 0)
    try:
        a = d.eff_lens(c, T, R); b = e.eff_lens(c, T, R)
    finally:
        d.close(); e.close()
    assert a.tobytes() == b.tobytes() == ps.eff_lens(w["lens"], c, R).tobytes()


def test_ratios_of_the_library():
    import rapmap_amd as ra
    ps.check_ratios(ra.pos_bias_ratios)


def test_host_arrays_beyond_one_part(crafted):
    """(1 << 21) + 65 hits through add_hits: one more than a part of host arrays takes, so the driver uploads and sweeps twice"""
    off, h = pc.big_batch()
    h = h.copy()
    rng = np.random.default_rng(8)
    w = crafted["world"]; T = w["lens"].size
    h["tid"] = rng.integers(0, T + 1, h.size); h["pos"] = rng.integers(-5, 200, h.size); h["mate_pos"] = rng.integers(-5, 200, h.size)
    h["frag_len"] = rng.integers(0, 140, h.size)
    f = _new(crafted["mp"])(100, 0)
    try:
        f.add_hits(off, h)
        c, s = f.counts(), f.stat()
    finally:
        f.close()
    # the restatement's loop over two million records would take a minute: the same rules in numpy, held to classify() on a slice
    eo, es = _classify_fast(w, off, h, 100)
    so, ss = ps.classify(w, off[:3001], h, 100); fo, fs = _classify_fast(w, off[:3001], h, 100)
    assert np.array_equal(so, fo) and ss == fs
    ps.assert_same(c, s, eo, es, "2 097 217 hits")
    assert s["folds"] == 2 and es["used"] > 1000 and es["overhang"] > 1000 and es["out_of_range"] > 1000


def _classify_fast(world, off, hits, max_len):
    """psb_cases.classify with the loop over the used records in numpy (int64 throughout: 20 x stays far below 2^63)"""
    off = np.asarray(off, dtype=np.int64); cnt = np.diff(off); n = cnt.size
    st = dict.fromkeys(ps.STATS, 0); st["units"] = n
    st["unmapped"] = int((cnt == 0).sum()); st["multi"] = int((cnt >= 2).sum())
    h = np.asarray(hits)[off[:-1][cnt == 1]]
    fl = h["frag_len"].astype(np.int64)
    npair = h["mate_status"] != 3; same = ~npair & (h["fwd"] == h["mate_is_fwd"]); oor = ~npair & ~same & ((fl == 0) | (fl > max_len))
    rest = ~npair & ~same & ~oor
    st["not_paired"] = int(npair.sum()); st["same_strand"] = int(same.sum()); st["out_of_range"] = int(oor.sum())
    h = h[rest]; fl = fl[rest]
    T = world["lens"].size
    tid = h["tid"].astype(np.int64); s = np.minimum(np.maximum(h["pos"].astype(np.int64), 0), np.maximum(h["mate_pos"].astype(np.int64), 0)); e = s + fl
    known = tid < T
    L = np.where(known, world["lens"][np.where(known, tid, 0)], -1)
    on = known & (e <= L)
    st["overhang"] = int((~on).sum()); st["used"] = int(on.sum())
    L = L[on]; s = s[on]; i = e[on] - 1
    c = np.searchsorted(np.array(ps.BOUNDS), L, side="left")
    obs = np.zeros(ps.SHAPE, dtype=np.uint64)
    np.add.at(obs[0], (c, (20 * s) // L), np.uint64(1)); np.add.at(obs[1], (c, (20 * i) // L), np.uint64(1))
    return obs, st


def test_times_and_errors(crafted):
    import rapmap_amd as ra
    mp = crafted["mp"]
    for bad, code in ((0, "-1"), (-5, "-1"), (1024, "-4")):         # QM_E_ARG, QM_E_ARG, QM_E_UNSUPPORTED
        with pytest.raises(ra.QmError, match=code):
            ra.PosBias(mp, max_len=bad)
    fresh = ra.QuasiMapper(crafted["qi"], 0)
    g = ra.PosBias(fresh)
    with pytest.raises(ra.QmError, match="-7"):                     # QM_E_STATE: no result yet
        g.add(fresh)
    with pytest.raises(ra.QmError, match="-1"):
        g.add_hits([0, 2, 1], np.zeros(2, dtype=ra.HIT_DTYPE))      # offsets that decrease
    assert all(v == 0 for k, v in g.stat().items() if k != "max_len")
    w = crafted["world"]; T = w["lens"].size
    off, h = gc.random_batch(w, 500, 1000, seed=1)
    g.add_hits(off, h)
    c = gc.histograms(w, 1000)["sparse"]
    g.expect(c, T, np.ones(T, dtype=np.uint64))
    g.eff_lens(c, T, np.ones(ps.SHAPE))
    s = g.stat()
    assert s["last_fold_us"] > 0 and s["last_expect_us"] > 0 and s["last_efflen_us"] > 0 and s["folds"] == 1
    g.close(); fresh.close()


@pytest.fixture(scope="module")
def small(synth_small):
    import rapmap_amd as ra
    qi = ra.QuasiIndex(synth_small["idx"])
    mp = ra.QuasiMapper(qi, 0, debug=False)
    q1, o1 = pack(synth_small["reads1"]); q2, o2 = pack(synth_small["reads2"])
    yield {"qi": qi, "mp": mp, "q1": q1, "o1": o1, "q2": q2, "o2": o2, "world": _world_of(qi)}
    mp.close()


@pytest.fixture(scope="module")
def oracle_small(small, synth_small, oracle_mod):
    """the oracle's hits of synth_small restated: fragment lengths and observed counts (shared; never changed)"""
    ix, orc = load_oracle(synth_small["idx"])
    res = orc.map_pairs(small["q1"], small["o1"], small["q2"], small["o2"], nthreads=4)
    counts, _ = fc.classify(res.hit_offsets, res.hits, 1000)
    obs, st = ps.classify(small["world"], res.hit_offsets, res.hits, 1000)
    for a in (counts, obs):
        a.setflags(write=False)
    return {"counts": counts, "obs": obs, "stats": st}


def test_synth_small_pairs(small, oracle_small):
    """the mapper's own result swept where it lies, against the oracle's hits; then the whole correction on that run's numbers"""
    import rapmap_amd as ra
    mp, w = small["mp"], small["world"]
    eo, es, counts = oracle_small["obs"], oracle_small["stats"], oracle_small["counts"]
    mp.map_pairs(small["q1"], small["o1"], small["q2"], small["o2"])
    g = ra.PosBias(mp)
    g.add(mp)
    ps.assert_same(g.counts(), g.stat(), eo, es, "synth_small: the oracle's hits")
    assert es["units"] == 4234 and es["used"] >= 500 and g.stat()["folds"] == 1 and g.stat()["last_fold_us"] > 0
    T = w["lens"].size
    alpha = np.random.default_rng(5).random(T) * 50
    q, k = ra.seq_bias_weights(alpha, w["lens"], counts)
    ex = g.expect(counts, T, q)
    exp, total = ps.expect(w, counts, q)
    assert np.array_equal(ex, exp)
    ps.assert_two_ends(ex, total, "synth_small")
    R = ra.pos_bias_ratios(g.counts(), ex)
    assert R.tobytes() == ps.ratios(eo, exp).tobytes()
    assert g.eff_lens(counts, T, R).tobytes() == ps.eff_lens(w["lens"], counts, R).tobytes()
    g.close()


def test_another_index_is_refused(small, crafted):
    import rapmap_amd as ra
    small["mp"].map_pairs(small["q1"], small["o1"], small["q2"], small["o2"])
    g = ra.PosBias(crafted["mp"])
    with pytest.raises(ra.QmError, match="-1"):                     # QM_E_ARG: the object holds another index's transcripts
        g.add(small["mp"])
    g.close()


# ---- the stream and the CLI on synth_small

@pytest.fixture(scope="module")
def small_fastq(synth_small, tmp_path_factory):
    d = tmp_path_factory.mktemp("psb_fq")
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
    with pytest.raises(ra.QmError, match="-7"):                   # QM_E_STATE: opened without pos_bias
        plain.pos_bias()
    assert plain.stats()["psb_sweep_s"] == 0
    plain.close()
    for classes in (False, True):
        st = ra.MappedStream(small["qi"], f1, f2, batch_units=512, threads=3, names=False, eq_classes=classes, hits=not classes, frag_len_dist=classes, pos_bias=True)
        with pytest.raises(ra.QmError, match="-7"):               # QM_E_STATE: the input has not ended
            st.pos_bias()
        nb = 0; per_batch = np.zeros(ps.SHAPE, dtype=np.uint64)
        for b in st:
            nb += 1
            if not classes:
                per_batch += ps.classify(small["world"], b.hit_offsets, b.hits, 1000)[0]
        obs, stats = st.pos_bias()
        assert nb == 9 and st.stats()["psb_sweep_s"] > 0 and st.stats()["sqb_sweep_s"] == 0 and st.stats()["gcb_sweep_s"] == 0
        ps.assert_same(obs, stats, oracle_small["obs"], oracle_small["stats"], "stream, eq_classes=%s" % classes)
        if classes:
            for x, y in zip(st.eq_classes(), table):
                assert x.tobytes() == y.tobytes()                 # the same class table with and without the sweep
            assert np.array_equal(st.frag_len_dist()[0], oracle_small["counts"])
        else:
            assert np.array_equal(per_batch, obs)                 # the sum over its batches
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


def test_cli_quant_pos_bias(small, synth_small, oracle_small, tmp_path):
    import rapmap_amd as ra
    qf, plain = str(tmp_path / "q.sf"), str(tmp_path / "plain.sf")
    r = _cli(_small_args(synth_small) + ["--quant", qf, "--quantFLD", "--quantPosBias"])
    assert r.returncode == 0, r.stderr
    assert "positional bias: units 4234, used %d" % oracle_small["stats"]["used"] in r.stderr and "overhang %d" % oracle_small["stats"]["overhang"] in r.stderr
    names, lens, eff, tpm, reads = ra.read_quant(qf)
    w, counts, obs = small["world"], oracle_small["counts"], oracle_small["obs"]
    T = small["qi"].n_txps
    # by hand: the first estimate on the fragment-length effective lengths, the restated weights, expected counts, ratios and
    # effective lengths, a second estimate on those started from the first
    t = _table(small)
    q1 = ra.Quant(t, T, fc.eff_lens(counts, lens)); q1.run(); first = q1.fetch(); q1.close()
    q, k = sq.weights(first, lens, counts)
    exp = ps.expect(w, counts, q)[0]
    R = ps.ratios(obs, exp)
    exp_eff = ps.eff_lens(w["lens"], counts, R)
    assert eff.tobytes() == exp_eff.tobytes()                     # (write_quant prints repr, read_quant's float() gives every bit back)
    q2 = ra.Quant(t, T, exp_eff); q2.set_start(first); q2.run(); second = q2.fetch(); q2.close(); t.close()
    assert reads.tobytes() == second.tobytes()
    assert (R != 1.0).any() and not np.array_equal(first, second)
    o_, e_, r_ = ra.read_pos_bias(qf + ".posBias.txt")
    assert np.array_equal(o_, obs) and np.array_equal(e_, exp) and r_.tobytes() == R.tobytes()
    assert os.path.exists(qf + ".flenDist.txt")
    # without the flag: what --quantFLD wrote before, and no posBias file
    r = _cli(_small_args(synth_small) + ["--quant", plain, "--quantFLD"])
    assert r.returncode == 0, r.stderr
    assert "positional bias" not in r.stderr and not os.path.exists(plain + ".posBias.txt")
    mine = str(tmp_path / "mine.sf")
    ra.write_quant(mine, small["qi"].txp_names, lens, fc.eff_lens(counts, lens), first)
    assert open(plain, "rb").read() == open(mine, "rb").read()
