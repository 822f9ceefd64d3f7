"""The fragment-length distribution on the device (qm_fld_*, MappedStream(frag_len_dist=True), quasimap --quantFLD) against the
restatement in fld_cases.py: classify() over the hits themselves, eff_lens() in float64.  Exact equality everywhere: integer counts,
and effective lengths bit for bit.  Run on the MI355X box: -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fld_cases as fc
import part_cases as pc
from conftest import GOLD, ROOT, load_oracle
from util import pack

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small(synth_small):
    import rapmap_amd as ra
    qi = ra.QuasiIndex(synth_small["idx"])
    mp = ra.QuasiMapper(qi, 0, debug=False)
    q1, o1 = pack(synth_small["reads1"]); q2, o2 = pack(synth_small["reads2"])
    yield {"qi": qi, "mp": mp, "q1": q1, "o1": o1, "q2": q2, "o2": o2}
    mp.close()


@pytest.fixture(scope="module")
def oracle_small(small, synth_small, oracle_mod):
    """the oracle's hits of synth_small per option set, and their restatement (shared; never changed)"""
    ix, orc = load_oracle(synth_small["idx"])
    out = {}
    for name, (oo, go) in SMALL_VARIANTS.items():
        res = orc.map_pairs(small["q1"], small["o1"], small["q2"], small["o2"], opts=oracle_mod.default_opts(**oo), nthreads=4)
        out[name] = fc.classify(res.hit_offsets, res.hits, 1000)
    rs = orc.map_single(small["q1"], small["o1"], nthreads=4)
    out["single"] = fc.classify(rs.hit_offsets, rs.hits, 1000)
    return out


def _new(mp):
    import rapmap_amd as ra
    return lambda max_len, max_blocks: ra.FragLenDist(mp, max_len=max_len, max_blocks=max_blocks)


@pytest.mark.parametrize("check", sorted(fc.CHECKS))
def test_crafted(small, check):
    fc.CHECKS[check](_new(small["mp"]))


def test_host_arrays_beyond_one_part(small):
    """(1 << 21) + 65 hits through add_hits: one more than a part of host arrays takes, so the driver uploads and folds twice.  (The
    cap of qm_eqc_add_labels, 1 << 25 tids, is crossed under the emulation only, at a cap of 5: test_eq_classes.py.)"""
    off, h = pc.big_batch()
    f = _new(small["mp"])(1000, 0)
    try:
        f.add_hits(off, h)
        c, s = f.counts(), f.stat()
    finally:
        f.close()
    ec, es = fc.classify(off, h, 1000)
    fc.assert_same(c, s, ec, es, "2 097 217 hits")
    assert s["folds"] == 2 and es["used"] > 10000 and es["out_of_range"] > 1000


SMALL_VARIANTS = {"default": ({}, {}), "fuzzy": ({"fuzzy": 1}, {"fuzzy": 1}), "no_dovetail": ({"noDovetail": 1}, {"no_dovetail": 1}),
                  "sel_aln": ({"selAln": 1}, {"sel_aln": 1})}


@pytest.mark.parametrize("variant", sorted(SMALL_VARIANTS))
def test_synth_small_pairs(small, oracle_small, variant):
    import rapmap_amd as ra
    mp = small["mp"]
    mp.map_pairs(small["q1"], small["o1"], small["q2"], small["o2"], opts=ra.default_opts(**SMALL_VARIANTS[variant][1]))
    f = ra.FragLenDist(mp)
    f.add(mp)
    ec, es = oracle_small[variant]
    fc.assert_same(f.counts(), f.stat(), ec, es, variant + ": the oracle's hits")
    assert es["units"] == 4234 and (variant != "default" or es["used"] >= 500)
    assert f.stat()["folds"] == 1 and f.stat()["last_fold_us"] > 0
    assert f.eff_lens(small["qi"].txp_lens).tobytes() == fc.eff_lens(ec, small["qi"].txp_lens).tobytes()
    assert f.mean() == ra.frag_len_mean(ec)
    f.close()


def test_synth_small_single_end(small, oracle_small):
    import rapmap_amd as ra
    mp = small["mp"]
    mp.map_reads(small["q1"], small["o1"])
    f = ra.FragLenDist(mp)
    f.add(mp)
    ec, es = oracle_small["single"]
    fc.assert_same(f.counts(), f.stat(), ec, es, "single-end: the oracle's hits")
    assert es["used"] == 0 and es["not_paired"] + es["unmapped"] + es["multi"] == es["units"] and es["not_paired"] > 500
    assert np.isnan(f.mean())
    f.close()


def test_sample_data(sample_data, oracle_mod):
    import rapmap_amd as ra
    qi = ra.QuasiIndex(sample_data["idx"])
    mp = ra.QuasiMapper(qi, 0)
    q1, o1 = pack(sample_data["reads1"]); q2, o2 = pack(sample_data["reads2"])
    mp.map_pairs(q1, o1, q2, o2)
    f = ra.FragLenDist(mp)
    f.add(mp)
    ix, orc = load_oracle(sample_data["idx"])
    res = orc.map_pairs(q1, o1, q2, o2, nthreads=4)
    ec, es = fc.classify(res.hit_offsets, res.hits, 1000)
    fc.assert_same(f.counts(), f.stat(), ec, es, "sample_data: the oracle's hits")
    assert es["used"] >= 5000
    f.close(); mp.close()


def test_repeat_families(repeat_data):
    """nearly every unit maps to many transcripts: multi"""
    import rapmap_amd as ra
    qi = ra.QuasiIndex(repeat_data["idx"])
    mp = ra.QuasiMapper(qi, 0, debug=False)
    q1, o1 = pack(repeat_data["reads1"]); q2, o2 = pack(repeat_data["reads2"])
    mp.map_pairs(q1, o1, q2, o2, opts=ra.default_opts(max_num_hits=2000))
    f = ra.FragLenDist(mp, max_blocks=1)
    f.add(mp)
    ix, orc = load_oracle(repeat_data["idx"])
    from oracle import oracle
    res = orc.map_pairs(q1, o1, q2, o2, opts=oracle.default_opts(maxNumHits=2000), nthreads=4)
    eo, so = fc.classify(res.hit_offsets, res.hits, 1000)
    fc.assert_same(f.counts(), f.stat(), eo, so, "repeat families: the oracle's hits")
    assert so["multi"] > 30 and int(np.diff(res.hit_offsets).max()) >= 900
    f.close(); mp.close()


def test_split_call(synth_medium, monkeypatch):
    """qm_map_device mapping the batch in parts leaves the same histogram as the unsplit call"""
    import torch
    import rapmap_amd as ra
    qi = ra.QuasiIndex(synth_medium["idx"])
    mp = ra.QuasiMapper(qi, 0, debug=False)
    n = 20001
    o = synth_medium["off"][: n + 1]
    q1 = synth_medium["seq1"][: o[-1]]; q2 = synth_medium["seq2"][: o[-1]]
    pad = np.zeros(8, np.uint8)
    d1 = torch.from_numpy(np.concatenate([q1, pad])).cuda(); d2 = torch.from_numpy(np.concatenate([q2, pad])).cuda(); do = torch.from_numpy(o).cuda()
    torch.cuda.synchronize()
    monkeypatch.setenv("QM_SPLIT", "1")
    whole = mp.map_device(n, d1.data_ptr(), do.data_ptr(), d2.data_ptr(), do.data_ptr(), 100, fetch=True)
    assert mp.stat(ra.QM_STAT_PAIR_KERNEL_PAIRS) == n                                        # QM_STAT_PAIR_KERNEL_PAIRS: one unsplit call over all pairs
    a = ra.FragLenDist(mp); a.add(mp)
    monkeypatch.setenv("QM_SPLIT_MIN", "1000"); monkeypatch.setenv("QM_SPLIT", "3")
    mp.map_device(n, d1.data_ptr(), do.data_ptr(), d2.data_ptr(), do.data_ptr(), 100, fetch=False)
    assert mp.stat(ra.QM_STAT_PAIR_KERNEL_PAIRS) == -1                                       # ... which a call mapped in parts reports as -1 (qmap_mi355.h)
    b = ra.FragLenDist(mp); b.add(mp)
    ec, es = fc.classify(whole.hit_offsets, whole.hits, 1000)
    fc.assert_same(a.counts(), a.stat(), ec, es, "device-resident, unsplit")
    fc.assert_same(b.counts(), b.stat(), ec, es, "device-resident, in parts")
    assert es["used"] > 0 and es["multi"] > 0 and es["units"] == n
    a.close(); b.close(); mp.close()


@pytest.fixture(scope="module")
def small_fastq(synth_small, tmp_path_factory):
    d = tmp_path_factory.mktemp("fld_fq")
    f1, f2 = str(d / "r1.fastq"), str(d / "r2.fastq")
    for fn, nms, rds in ((f1, synth_small["names1"], synth_small["reads1"]), (f2, synth_small["names2"], synth_small["reads2"])):
        with open(fn, "wb") as fh:
            for nm, r in zip(nms, rds):
                fh.write(b"@" + nm.encode() + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
    return f1, f2


def test_stream(small, oracle_small, small_fastq):
    import rapmap_amd as ra
    ec, es = oracle_small["default"]
    f1, f2 = small_fastq
    plain = ra.MappedStream(small["qi"], f1, f2, batch_units=512, threads=3, names=False, eq_classes=True, hits=False)
    for b in plain:
        pass
    table = plain.eq_classes()
    with pytest.raises(ra.QmError, match="-7"):                   # QM_E_STATE: opened without frag_len_dist
        plain.frag_len_dist()
    assert plain.stats()["fld_fold_s"] == 0
    plain.close()
    for classes in (False, True):
        st = ra.MappedStream(small["qi"], f1, f2, batch_units=512, threads=3, names=False, eq_classes=classes, hits=not classes, frag_len_dist=True)
        with pytest.raises(ra.QmError, match="-7"):               # QM_E_STATE: the input has not ended
            st.frag_len_dist()
        nb = 0
        for b in st:
            nb += 1
            assert (b.hits is None) == classes
        counts, stats = st.frag_len_dist()
        assert nb == 9 and st.stats()["fld_fold_s"] > 0            # 4 234 pairs in batches of 512: every context folded some
        fc.assert_same(counts, stats, ec, es, "stream, eq_classes=%s" % classes)
        if classes:
            for x, y in zip(st.eq_classes(), table):
                assert x.tobytes() == y.tobytes()
        st.close()


def test_errors(small):
    import rapmap_amd as ra
    for bad, code in ((0, "-1"), (-5, "-1"), (1024, "-4")):       # QM_E_ARG, QM_E_ARG, QM_E_UNSUPPORTED
        with pytest.raises(ra.QmError, match=code):
            ra.FragLenDist(small["mp"], max_len=bad)
    fresh = ra.QuasiMapper(small["qi"], 0)
    f = ra.FragLenDist(fresh)
    with pytest.raises(ra.QmError, match="-7"):                   # QM_E_STATE: no result yet
        f.add(fresh)
    with pytest.raises(ra.QmError, match="-1"):
        f.add_hits([0, 2, 1], np.zeros(2, dtype=ra.HIT_DTYPE))    # offsets that decrease
    assert all(v == 0 for k, v in f.stat().items() if k != "max_len")
    f.close(); fresh.close()


def test_across_devices(small):
    import torch
    import rapmap_amd as ra
    if torch.cuda.device_count() < 2:
        pytest.skip("one device: the cross-device check needs two")
    other = ra.QuasiMapper(small["qi"], 1)
    g = ra.FragLenDist(other)
    small["mp"].map_pairs(small["q1"], small["o1"], small["q2"], small["o2"])
    with pytest.raises(ra.QmError, match="-1"):                   # QM_E_ARG: histogram and context on different devices
        g.add(small["mp"])
    g.close(); other.close()


# ---- the CLI on synth_small

def _cli(args):
    return subprocess.run([sys.executable, "-m", "rapmap_amd", "quasimap"] + args, cwd=ROOT, capture_output=True, text=True)


def _small_args(synth_small):
    sd = os.path.join(GOLD, "synth_small")
    return ["-i", synth_small["idx"], "-1", os.path.join(sd, "reads_1.fastq.gz"), "-2", os.path.join(sd, "reads_2.fastq.gz"), "-t", "4", "-n"]


def _alpha_by_hand(small, eff):
    """a Quant run on a table filled the way the CLI fills its own (a table of the default size, the sorted classes in one add_labels:
    equal input gives equal slots, hence the same order of every sum)"""
    import rapmap_amd as ra
    mp = small["mp"]
    mp.map_pairs(small["q1"], small["o1"], small["q2"], small["o2"])
    src = ra.EqClasses(mp); src.add(mp)
    t = ra.EqClasses(mp); t.add_labels(*src.fetch())
    q = ra.Quant(t, small["qi"].n_txps, eff)
    q.run()
    alpha = q.fetch()
    q.close(); t.close(); src.close()
    return alpha


def test_cli_quant_fld(small, synth_small, oracle_small, tmp_path):
    import rapmap_amd as ra
    ec, es = oracle_small["default"]
    qf = str(tmp_path / "q.sf")
    r = _cli(_small_args(synth_small) + ["--quant", qf, "--quantFLD"])
    assert r.returncode == 0, r.stderr
    assert "fragment lengths: mean" in r.stderr and "used %d" % es["used"] in r.stderr and "multi %d" % es["multi"] in r.stderr
    dist_ = ra.read_flen_dist(qf + ".flenDist.txt")
    assert dist_.size == 1001 and np.array_equal(np.rint(dist_ * es["used"]).astype(np.uint64), ec)
    names, lens, eff, tpm, reads = ra.read_quant(qf)
    assert names == small["qi"].txp_names and np.array_equal(lens, small["qi"].txp_lens)
    # write_quant prints floats with repr, which read_quant's float() gives back bit for bit: the comparison is of all 64 bits
    exp = fc.eff_lens(ec, lens)
    assert eff.tobytes() == exp.tobytes()
    assert (exp < lens).any() and (exp >= 1).all()
    assert reads.tobytes() == _alpha_by_hand(small, exp).tobytes()
    assert abs(float(tpm.sum()) - 1e6) <= 1e-6
    assert not os.path.exists(qf + ".bootstraps.gz")


def test_cli_quant_fld_bootstraps(small, synth_small, tmp_path):
    import rapmap_amd as ra
    qf = str(tmp_path / "q.sf")
    r = _cli(_small_args(synth_small) + ["-q", "--quant", qf, "--quantFLD", "--numBootstraps", "3"])
    assert r.returncode == 0, r.stderr
    assert os.path.exists(qf + ".flenDist.txt")
    assert ra.read_bootstraps(qf + ".bootstraps.gz", small["qi"].n_txps).shape == (3, small["qi"].n_txps)


def test_cli_without_the_flag_is_unchanged(small, synth_small, tmp_path):
    """no --quantFLD: the lengths are the effective lengths, as before, and nothing else is written"""
    import rapmap_amd as ra
    qf, mine = str(tmp_path / "q.sf"), str(tmp_path / "mine.sf")
    r = _cli(_small_args(synth_small) + ["--quant", qf])
    assert r.returncode == 0, r.stderr
    assert "fragment lengths" not in r.stderr and not os.path.exists(qf + ".flenDist.txt")
    lens = np.asarray(small["qi"].txp_lens, dtype=np.int64)
    eff = np.maximum(1.0, lens.astype(np.float64))
    ra.write_quant(mine, small["qi"].txp_names, lens, eff, _alpha_by_hand(small, eff))
    assert open(qf, "rb").read() == open(mine, "rb").read()


@pytest.mark.parametrize("case", ["no_quant", "frag_len_mean", "single_end"])
def test_cli_rejects(synth_small, tmp_path, case):
    a = _small_args(synth_small)
    qf = str(tmp_path / "q.sf")
    if case == "no_quant":
        args, why = a + ["--quantFLD"], "needs --quant"
    elif case == "frag_len_mean":
        args, why = a + ["--quant", qf, "--quantFLD", "--quantFragLenMean", "200"], "not together with"
    else:
        args, why = ["-i", synth_small["idx"], "-r", a[3], "-n", "--quant", qf, "--quantFLD"], "needs paired-end reads"
    r = _cli(args)
    assert r.returncode != 0 and "--quantFLD" in r.stderr and why in r.stderr and not os.path.exists(qf)
