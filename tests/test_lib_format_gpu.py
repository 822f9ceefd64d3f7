"""The library type on the device (qm_lib_*, qm_eqc_add_lib, MappedStream(lib_type=...), quasimap --libType) against the restatement in
lib_cases.py: codes(), tally() and filtered_classes() over the hits themselves.  Exact equality everywhere: integer tallies, offsets,
tid lists, class tables.  Run on the MI355X box: -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lib_cases as lc
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


SMALL_VARIANTS = {"default": ({}, {}), "fuzzy": ({"fuzzy": 1}, {"fuzzy": 1}), "no_dovetail": ({"noDovetail": 1}, {"no_dovetail": 1}),
                  "sel_aln": ({"selAln": 1}, {"sel_aln": 1})}


@pytest.fixture(scope="module")
def oracle_small(small, synth_small, oracle_mod):
    """the oracle's hits of synth_small per option set (shared; never changed)"""
    ix, orc = load_oracle(synth_small["idx"])
    out = {}
    for name, (oo, go) in SMALL_VARIANTS.items():
        res = orc.map_pairs(small["q1"], small["o1"], small["q2"], small["o2"], opts=oracle_mod.default_opts(**oo), nthreads=4)
        out[name] = (res.hit_offsets, res.hits)
    rs = orc.map_single(small["q1"], small["o1"], nthreads=4)
    out["single"] = (rs.hit_offsets, rs.hits)
    return out


def _new(mp):
    import rapmap_amd as ra
    return lambda lib_type, max_blocks: ra.LibFormat(mp, lib_type, max_blocks=max_blocks)


@pytest.mark.parametrize("check", sorted(lc.CHECKS))
def test_crafted(small, check):
    lc.CHECKS[check](_new(small["mp"]))


def test_host_arrays_beyond_one_part(small):
    """(1 << 21) + 65 hits through add_hits and compact_hits ("ISF"): one more than a part of host arrays takes, so the driver uploads
    and sweeps twice and joins the two parts' filtered lists.  (The cap of qm_eqc_add_labels, 1 << 25 tids, is crossed under the
    emulation only, at a cap of 5: test_eq_classes.py.)"""
    off, h = pc.big_batch()
    ew, eo, et = lc.tally(off, h, "ISF")
    a = _new(small["mp"])("ISF", 0); b = _new(small["mp"])("ISF", 0)
    try:
        a.add_hits(off, h)
        no, t = b.compact_hits(off, h)
        lc.assert_same(a.counts(), ew, "ISF", "2 097 217 hits (add_hits)"); lc.assert_same(b.counts(), ew, "ISF", "2 097 217 hits (compact_hits)")
        assert np.array_equal(no, eo) and np.array_equal(t, et)
        assert a.stat()["sweeps"] == 2 and b.stat()["sweeps"] == 2
        assert int(ew[lc.W_KEPT_HITS]) > 100000 and int(ew[lc.W_DROPPED]) > 1000
    finally:
        a.close(); b.close()


def _fold(mp, lib_type, max_blocks=0):
    """EqClasses.add(mapper, lib) over the mapper's last result -> (table, tallies, stat)"""
    import rapmap_amd as ra
    lib = ra.LibFormat(mp, lib_type, max_blocks=max_blocks); t = ra.EqClasses(mp, expected=64)
    try:
        t.add(mp, lib=lib)
        return t.fetch(), lib.counts(), lib.stat()
    finally:
        t.close(); lib.close()


@pytest.mark.parametrize("variant", sorted(SMALL_VARIANTS))
def test_synth_small_pairs(small, oracle_small, variant):
    import rapmap_amd as ra
    mp = small["mp"]
    mp.map_pairs(small["q1"], small["o1"], small["q2"], small["o2"], opts=ra.default_opts(**SMALL_VARIANTS[variant][1]))
    off, hits = oracle_small[variant]
    plain = ra.EqClasses(mp, expected=64); plain.add(mp)
    for t in ("ISF", "ISR", "IU", "A"):
        ew, eo, et = lc.tally(off, hits, t)
        f = ra.LibFormat(mp, t); f.add(mp)
        lc.assert_same(f.counts(), ew, t, "%s, %s: the oracle's hits" % (variant, t))
        assert f.stat()["sweeps"] == 1 and f.stat()["last_sweep_us"] > 0 and f.stat()["mask"] == lc.mask_of(t)
        f.close()
        table, ctr, st = _fold(mp, t)
        lc.assert_same(ctr, ew, t, "%s, %s: qm_eqc_add_lib's tallies" % (variant, t))
        if t == "A":
            for x, y in zip(table, plain.fetch()):
                assert x.tobytes() == y.tobytes()
        else:
            assert lc.table_classes(*table) == lc.filtered_classes(eo, et), (variant, t)
        assert int(ew[lc.W_UNITS]) == 4234
        if variant == "default" and t in ("ISF", "ISR"):
            assert int(ew[lc.W_KEPT]) >= 1500 and int(ew[lc.W_DROPPED]) >= 1500
    if variant == "default":
        assert ra.infer_lib_type(ew) == "IU" == lc.infer(ew)
    plain.close()


def test_synth_small_single_end(small, oracle_small):
    """a single-end call is tallied in codes 10 and 11 only, and U keeps all of it"""
    import rapmap_amd as ra
    mp = small["mp"]
    mp.map_reads(small["q1"], small["o1"])
    off, hits = oracle_small["single"]
    ew, eo, et = lc.tally(off, hits, "U")
    table, ctr, st = _fold(mp, "U")
    lc.assert_same(ctr, ew, "U", "single-end")
    assert int(ew[:10].sum()) == 0 and int(ew[lc.SF]) > 500 and int(ew[lc.SR]) > 500 and int(ew[lc.W_KEPT_HITS]) == int(ew[lc.W_HITS]) == len(hits)
    plain = ra.EqClasses(mp, expected=64); plain.add(mp)
    for x, y in zip(table, plain.fetch()):
        assert x.tobytes() == y.tobytes()
    plain.close()
    assert ra.infer_lib_type(ew) == lc.infer(ew) in ("U", "SF", "SR")


def test_sample_data(sample_data, oracle_mod):
    import rapmap_amd as ra
    qi = ra.QuasiIndex(sample_data["idx"])
    mp = ra.QuasiMapper(qi, 0)
    q1, o1 = pack(sample_data["reads1"]); q2, o2 = pack(sample_data["reads2"])
    mp.map_pairs(q1, o1, q2, o2)
    ix, orc = load_oracle(sample_data["idx"])
    res = orc.map_pairs(q1, o1, q2, o2, nthreads=4)
    for t in ("ISF", "ISR"):
        ew, eo, et = lc.tally(res.hit_offsets, res.hits, t)
        table, ctr, st = _fold(mp, t, max_blocks=1)
        lc.assert_same(ctr, ew, t, "sample_data: the oracle's hits")
        assert lc.table_classes(*table) == lc.filtered_classes(eo, et)
        assert int(ew[lc.W_KEPT]) >= 4000 and int(ew[lc.W_DROPPED]) >= 4000
    assert ra.infer_lib_type(ew) == "IU"
    mp.close()


def test_split_call(synth_medium, monkeypatch):
    """qm_map_device mapping the batch in parts leaves the same tallies and the same filtered classes as the unsplit call"""
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
    ta, ca, _ = _fold(mp, "ISF")
    monkeypatch.setenv("QM_SPLIT_MIN", "1000"); monkeypatch.setenv("QM_SPLIT", "3")
    mp.map_device(n, d1.data_ptr(), do.data_ptr(), d2.data_ptr(), do.data_ptr(), 100, fetch=False)
    assert mp.stat(ra.QM_STAT_PAIR_KERNEL_PAIRS) == -1                                       # mapped in parts
    tb, cb, _ = _fold(mp, "ISF")
    ew, eo, et = lc.tally(whole.hit_offsets, whole.hits, "ISF")
    lc.assert_same(ca, ew, "ISF", "device-resident, unsplit"); lc.assert_same(cb, ew, "ISF", "device-resident, in parts")
    exp = lc.filtered_classes(eo, et)
    assert lc.table_classes(*ta) == exp == lc.table_classes(*tb)
    assert int(ew[lc.W_KEPT]) > 1000 and int(ew[lc.W_DROPPED]) > 1000 and int(ew[lc.W_UNITS]) == n
    mp.close()


@pytest.fixture(scope="module")
def small_fastq(synth_small, tmp_path_factory):
    d = tmp_path_factory.mktemp("lib_fq")
    f1, f2 = str(d / "r1.fastq"), str(d / "r2.fastq")
    for fn, nms, rds in ((f1, synth_small["names1"], synth_small["reads1"]), (f2, synth_small["names2"], synth_small["reads2"])):
        with open(fn, "wb") as fh:
            for nm, r in zip(nms, rds):
                fh.write(b"@" + nm.encode() + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
    return f1, f2


def test_stream(small, oracle_small, small_fastq):
    import rapmap_amd as ra
    off, hits = oracle_small["default"]
    ew, eo, et = lc.tally(off, hits, "ISF")
    f1, f2 = small_fastq
    plain = ra.MappedStream(small["qi"], f1, f2, batch_units=512, threads=3, names=False)
    for b in plain:
        pass
    with pytest.raises(ra.QmError, match="-7"):                   # QM_E_STATE: opened without lib_type
        plain.lib_counts()
    plain.close()
    for classes in (False, True):
        st = ra.MappedStream(small["qi"], f1, f2, batch_units=512, threads=3, names=False, eq_classes=classes, hits=not classes, lib_type="ISF")
        with pytest.raises(ra.QmError, match="-7"):               # QM_E_STATE: the input has not ended
            st.lib_counts()
        nb = 0; per_batch = np.zeros(32, dtype=np.uint64)
        for b in st:
            nb += 1
            assert (b.hits is None) == classes
            if not classes:
                per_batch += lc.tally(b.hit_offsets, b.hits, "ISF")[0]
        assert nb == 9                                             # 4 234 pairs in batches of 512
        lc.assert_same(st.lib_counts(), ew, "ISF", "stream, eq_classes=%s" % classes)
        if classes:
            assert lc.table_classes(*st.eq_classes()) == lc.filtered_classes(eo, et)
        else:
            assert np.array_equal(per_batch, ew)                  # the tallies are the sum over the batches
        st.close()


def test_two_contexts_merged(small, oracle_small):
    """two contexts each take half of the pairs; add_counts and add_labels merge tallies and tables"""
    import rapmap_amd as ra
    off, hits = oracle_small["default"]
    ew, eo, et = lc.tally(off, hits, "ISR")
    other = ra.QuasiMapper(small["qi"], 0)
    n = len(small["o1"]) - 1; h = n // 2
    la = ra.LibFormat(small["mp"], "ISR"); lb = ra.LibFormat(other, "ISR"); ta = ra.EqClasses(small["mp"], expected=64); tb = ra.EqClasses(other, expected=64)
    o1, o2 = small["o1"], small["o2"]
    small["mp"].map_pairs(small["q1"][:o1[h]], o1[:h + 1], small["q2"][:o2[h]], o2[:h + 1])
    other.map_pairs(small["q1"][o1[h]:], o1[h:] - o1[h], small["q2"][o2[h]:], o2[h:] - o2[h])
    ta.add(small["mp"], lib=la); tb.add(other, lib=lb)
    la.add_counts(lb.counts()); ta.add_labels(*tb.fetch())
    lc.assert_same(la.counts(), ew, "ISR", "two contexts")
    assert lc.table_classes(*ta.fetch()) == lc.filtered_classes(eo, et)
    for x in (la, lb, ta, tb, other):
        x.close()


def test_errors(small):
    import rapmap_amd as ra
    for bad in (0, 0x1000, 0x10fff, 0xffffffff):
        with pytest.raises(ra.QmError, match="-1"):               # QM_E_ARG: no code, or a bit above 11
            ra.LibFormat(small["mp"], bad)
    with pytest.raises(ra.QmError, match="-1"):
        ra.LibFormat(small["mp"], "XX")
    fresh = ra.QuasiMapper(small["qi"], 0)
    f = ra.LibFormat(fresh, "IU"); t = ra.EqClasses(fresh, expected=64)
    with pytest.raises(ra.QmError, match="-7"):                   # QM_E_STATE: no result yet
        f.add(fresh)
    with pytest.raises(ra.QmError, match="-7"):
        t.add(fresh, lib=f)
    with pytest.raises(ra.QmError, match="-1"):
        f.add_hits([0, 2, 1], np.zeros(2, dtype=ra.HIT_DTYPE))    # offsets that decrease
    assert not f.counts().any() and f.stat()["sweeps"] == 0
    f.close(); t.close(); fresh.close()


def test_across_devices(small):
    import torch
    import rapmap_amd as ra
    if torch.cuda.device_count() < 2:
        pytest.skip("one device: the cross-device check needs two")
    other = ra.QuasiMapper(small["qi"], 1)
    g = ra.LibFormat(other, "IU"); t = ra.EqClasses(small["mp"], expected=64)
    small["mp"].map_pairs(small["q1"], small["o1"], small["q2"], small["o2"])
    with pytest.raises(ra.QmError, match="-1"):                   # QM_E_ARG: object and context on different devices
        g.add(small["mp"])
    with pytest.raises(ra.QmError, match="-1"):
        t.add(small["mp"], lib=g)
    g.close(); t.close(); other.close()


# ---- the CLI on synth_small

def _cli(args):
    return subprocess.run([sys.executable, "-m", "rapmap_amd", "quasimap"] + args, cwd=ROOT, capture_output=True, text=True)


def _small_args(synth_small):
    sd = os.path.join(GOLD, "synth_small")
    return ["-i", synth_small["idx"], "-1", os.path.join(sd, "reads_1.fastq.gz"), "-2", os.path.join(sd, "reads_2.fastq.gz"), "-t", "4", "-n"]


def test_cli_quant_lib_type(small, synth_small, oracle_small, tmp_path):
    """--quant --libType ISR: NumReads is a Quant run over the filtered classes (a table filled the way the CLI fills its own: the
    sorted classes in one add_labels), the JSON holds the tallies"""
    import rapmap_amd as ra
    off, hits = oracle_small["default"]
    ew, eo, et = lc.tally(off, hits, "ISR")
    qf = str(tmp_path / "q.sf")
    r = _cli(_small_args(synth_small) + ["--quant", qf, "--libType", "ISR"])
    assert r.returncode == 0, r.stderr
    assert "library type ISR" in r.stderr and "%d dropped" % int(ew[lc.W_DROPPED]) in r.stderr
    counts, d = ra.read_lib_format_counts(qf + ".lib_format_counts.json")
    lc.assert_same(counts, ew, "ISR", "the CLI's JSON")
    assert d["expected_format"] == "ISR" and d["inferred_format"] == "IU"
    mp = small["mp"]
    mp.map_pairs(small["q1"], small["o1"], small["q2"], small["o2"])
    lib = ra.LibFormat(mp, "ISR"); src = ra.EqClasses(mp); src.add(mp, lib=lib)
    t = ra.EqClasses(mp); t.add_labels(*src.fetch())
    lens = np.asarray(small["qi"].txp_lens, dtype=np.int64)
    q = ra.Quant(t, small["qi"].n_txps, np.maximum(1.0, lens.astype(np.float64)))
    q.run()
    alpha = q.fetch()
    q.close(); t.close(); src.close(); lib.close()
    names, lens2, eff, tpm, reads = ra.read_quant(qf)
    assert reads.tobytes() == alpha.tobytes()
    assert abs(float(reads.sum()) - int(ew[lc.W_KEPT])) < 1e-6 * int(ew[lc.W_KEPT])


def test_cli_lib_type_a_changes_nothing(synth_small, tmp_path):
    """--libType A drops nothing: quant.sf and the classes are byte-identical to a run without the flag, which writes no JSON"""
    qa, qb, ea, eb = (str(tmp_path / x) for x in ("a.sf", "b.sf", "a.eq", "b.eq"))
    r = _cli(_small_args(synth_small) + ["--quant", qa, "--eqClasses", ea, "--libType", "A"])
    assert r.returncode == 0, r.stderr
    assert "the single-hit units point to IU" in r.stderr and os.path.exists(ea + ".lib_format_counts.json")
    r = _cli(_small_args(synth_small) + ["--quant", qb, "--eqClasses", eb])
    assert r.returncode == 0, r.stderr
    assert "library type" not in r.stderr and not os.path.exists(eb + ".lib_format_counts.json") and not os.path.exists(qb + ".lib_format_counts.json")
    assert open(qa, "rb").read() == open(qb, "rb").read() and open(ea, "rb").read() == open(eb, "rb").read()


@pytest.mark.parametrize("case", ["paired_type_single_end", "single_type_paired"])
def test_cli_rejects(synth_small, tmp_path, case):
    a = _small_args(synth_small)
    qf = str(tmp_path / "q.sf")
    if case == "paired_type_single_end":
        args, why = ["-i", synth_small["idx"], "-r", a[3], "-n", "--quant", qf, "--libType", "ISF"], "needs paired-end reads"
    else:
        args, why = a + ["--quant", qf, "--libType", "SF"], "not with paired-end reads"
    r = _cli(args)
    assert r.returncode != 0 and "--libType" in r.stderr and why in r.stderr and not os.path.exists(qf)
