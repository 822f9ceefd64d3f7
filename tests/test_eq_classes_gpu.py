"""Equivalence classes on the device (qm_eqc_*, MappedStream(eq_classes=True), quasimap --eqClasses) against dictionaries built here from
the lists / the hits themselves: tuple(sorted(set(tids))) -> count.  Exact equality of the three fetched arrays, no tolerance.
Run on the MI355X box: -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

import eqc_cases as ec
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
def crafted():
    L, w = ec.crafted_lists()
    off, tids = ec.csr(L)
    return L, w, off, tids


@pytest.fixture(scope="module")
def small_default(small):
    """the default mapping of synth_small, its table as a dictionary and as fetched arrays (shared; never changed)"""
    import rapmap_amd as ra
    gr = small["mp"].map_pairs(small["q1"], small["o1"], small["q2"], small["o2"])
    t = ra.EqClasses(small["mp"])
    t.add(small["mp"])
    got = t.fetch(); t.close()
    return gr, ec.expected_from_hits(gr.hit_offsets, gr.hits), got


@pytest.mark.parametrize("weights", [False, True])
def test_crafted_lists(small, crafted, weights):
    import rapmap_amd as ra
    L, w, off, tids = crafted
    assert len(L) > 2900 and [] in L and max(len(x) for x in L) > 2048
    ww = w if weights else None
    t = ra.EqClasses(small["mp"], expected=4096)
    t.add_labels(off, tids, ww)
    d = ec.expected(L, ww)
    ec.assert_table(t.fetch(), d, "crafted lists")
    assert t.total == sum((int(w[i]) if weights else 1) for i, x in enumerate(L) if len(x))
    assert t.n_classes == len(d)
    assert t.stat(t.LONG_UNITS) == sum(1 for x in L if len(x) > 8)
    t.close()


def test_forced_collisions(small):
    import rapmap_amd as ra
    L = ec.distinct_labels(500)
    off, tids = ec.csr(L)
    a = ra.EqClasses(small["mp"], expected=1024, hash_bits=0); a.add_labels(off, tids)
    b = ra.EqClasses(small["mp"], expected=1024, hash_bits=4); b.add_labels(off, tids)
    fa, fb = a.fetch(), b.fetch()
    ec.assert_table(fa, ec.expected(L), "all key bits")
    for x, y in zip(fa, fb):
        assert x.tobytes() == y.tobytes()
    assert b.stat(b.COLLISION_PROBES) > 0
    a.close(); b.close()


@pytest.mark.parametrize("folds", [1, 5])
def test_growth(small, folds):
    import rapmap_amd as ra
    L = ec.distinct_labels(5000)
    t = ra.EqClasses(small["mp"], expected=1)
    for f in range(folds):
        part = L[f * 5000 // folds:(f + 1) * 5000 // folds]
        t.add_labels(*ec.csr(part))
    assert t.stat(t.GROWTHS) > 0
    ec.assert_table(t.fetch(), ec.expected(L), "5 000 labels into a table made for one, %d folds" % folds)
    assert t.n_classes == 5000 and t.total == 5000
    t.close()


def test_accumulation_clear_and_determinism(small, crafted):
    import rapmap_amd as ra
    L, w, off, tids = crafted
    d = ec.expected(L, w)
    t = ra.EqClasses(small["mp"], expected=64)
    for _ in range(3):
        t.add_labels(off, tids, w)
    ec.assert_table(t.fetch(), {k: 3 * v for k, v in d.items()}, "three folds")
    t.clear()
    assert t.n_classes == 0 and t.total == 0 and t.fetch()[0].tolist() == [0]
    t.add_labels(off, tids, w)
    once = t.fetch()
    ec.assert_table(once, d, "after clear")
    u = ra.EqClasses(small["mp"], expected=1 << 16)
    u.add_labels(off, tids, w)
    for x, y in zip(once, u.fetch()):
        assert x.tobytes() == y.tobytes()
    t.close(); u.close()


def test_state_and_argument_errors(small):
    import rapmap_amd as ra
    fresh = ra.QuasiMapper(small["qi"], 0)
    t = ra.EqClasses(fresh)
    with pytest.raises(ra.QmError, match="-7"):                   # QM_E_STATE: no result yet
        t.add(fresh)
    with pytest.raises(ra.QmError, match="-1"):
        t.add_labels([0, 2, 1], [1, 2])                           # offsets that decrease
    t.close(); fresh.close()


SMALL_VARIANTS = {"default": ({}, {}), "fuzzy": ({"fuzzy": 1}, {"fuzzy": 1}), "sel_aln": ({"selAln": 1}, {"sel_aln": 1}),
                  "no_orphans": ({"noOrphans": 1}, {"no_orphans": 1})}


@pytest.mark.parametrize("variant", sorted(SMALL_VARIANTS))
def test_synth_small_pairs(small, synth_small, oracle_mod, variant):
    import rapmap_amd as ra
    oo, go = SMALL_VARIANTS[variant]
    mp = small["mp"]
    assert len(small["o1"]) - 1 == 4234
    gr = mp.map_pairs(small["q1"], small["o1"], small["q2"], small["o2"], opts=ra.default_opts(**go))
    t = ra.EqClasses(mp, expected=256)
    t.add(mp)
    got = t.fetch()
    ec.assert_table(got, ec.expected_from_hits(gr.hit_offsets, gr.hits), variant + ": the mapper's own hits")
    ix, orc = load_oracle(synth_small["idx"])
    res = orc.map_pairs(small["q1"], small["o1"], small["q2"], small["o2"], opts=oracle_mod.default_opts(**oo), nthreads=4)
    ec.assert_table(got, ec.expected_from_hits(res.hit_offsets, res.hits), variant + ": the oracle's hits")
    assert t.total == int(np.count_nonzero(np.diff(gr.hit_offsets)))
    t.close()


def test_synth_small_single_end(small, synth_small, oracle_mod):
    import rapmap_amd as ra
    mp = small["mp"]
    gr = mp.map_reads(small["q1"], small["o1"])
    t = ra.EqClasses(mp)
    t.add(mp)
    got = t.fetch()
    ec.assert_table(got, ec.expected_from_hits(gr.hit_offsets, gr.hits), "single-end: the mapper's own hits")
    ix, orc = load_oracle(synth_small["idx"])
    rs = orc.map_single(small["q1"], small["o1"], nthreads=4)
    ec.assert_table(got, ec.expected_from_hits(rs.hit_offsets, rs.hits), "single-end: the oracle's hits")
    assert t.total == int(np.count_nonzero(np.diff(gr.hit_offsets)))
    t.close()


@pytest.mark.parametrize("max_num_hits", [2000, 200])
def test_repeat_families(repeat_data, max_num_hits):
    import rapmap_amd as ra
    qi = ra.QuasiIndex(repeat_data["idx"])
    mp = ra.QuasiMapper(qi, 0, debug=False)
    q1, o1 = pack(repeat_data["reads1"]); q2, o2 = pack(repeat_data["reads2"])
    gr = mp.map_pairs(q1, o1, q2, o2, opts=ra.default_opts(max_num_hits=max_num_hits))
    t = ra.EqClasses(mp, expected=16)
    t.add(mp)
    d = ec.expected_from_hits(gr.hit_offsets, gr.hits)
    longest = max(len(k) for k in d)
    # the fixture's families: 40 copies fit -m 200; 300 and 900 copies need -m 2000; 1 100 copies are beyond maxInterval (1000) either way
    assert longest >= (900 if max_num_hits == 2000 else 40), longest
    ec.assert_table(t.fetch(), d, "repeat families, -m %d" % max_num_hits)
    assert t.stat(t.LONG_UNITS) > 0
    assert t.total == int(np.count_nonzero(np.diff(gr.hit_offsets)))
    t.close(); mp.close()


def test_split_call(synth_medium, monkeypatch):
    """qm_map_device mapping the batch in parts leaves the same table as the unsplit call"""
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
    a = ra.EqClasses(mp); a.add(mp)
    monkeypatch.setenv("QM_SPLIT_MIN", "1000"); monkeypatch.setenv("QM_SPLIT", "3")
    mp.map_device(n, d1.data_ptr(), do.data_ptr(), d2.data_ptr(), do.data_ptr(), 100, fetch=False)
    assert mp.stat(ra.QM_STAT_PAIR_KERNEL_PAIRS) == -1                                       # ... which a call mapped in parts reports as -1 (qmap_mi355.h)
    b = ra.EqClasses(mp); b.add(mp)
    fa = a.fetch()
    ec.assert_table(fa, ec.expected_from_hits(whole.hit_offsets, whole.hits), "device-resident, unsplit")
    for x, y in zip(fa, b.fetch()):
        assert x.tobytes() == y.tobytes()
    a.close(); b.close(); mp.close()


@pytest.fixture(scope="module")
def small_fastq(synth_small, tmp_path_factory):
    d = tmp_path_factory.mktemp("eqc_fq")
    f1, f2 = str(d / "r1.fastq"), str(d / "r2.fastq")
    for fn, nms, rds in ((f1, synth_small["names1"], synth_small["reads1"]), (f2, synth_small["names2"], synth_small["reads2"])):
        with open(fn, "wb") as fh:
            for nm, r in zip(nms, rds):
                fh.write(b"@" + nm.encode() + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
    return f1, f2


def test_stream(small, small_default, small_fastq):
    import rapmap_amd as ra
    gr, d, one_shot = small_default
    f1, f2 = small_fastq
    tots = []
    for hits in (True, False):
        st = ra.MappedStream(small["qi"], f1, f2, batch_units=500, threads=3, names=False, eq_classes=True, hits=hits)
        tot = {}; nb = 0; nh = 0
        for b in st:
            nb += 1; nh += b.n_hits
            if hits:
                assert b.hits.size == b.n_hits and b.hit_offsets.size == b.n + 1
            else:
                assert b.hits is None and b.hit_offsets is None
            for k, v in b.counters.items():
                tot[k] = tot.get(k, 0) + v
        got = st.eq_classes()
        ss = st.stats()
        st.close()
        assert ss["fold_contexts"] >= 2 and ss["fold_s"] > 0          # more than one context held a partial table: the merge had work
        assert nb == 9 and nh == gr.n_hits                        # 4 234 pairs in batches of 500: every context folded some
        ec.assert_table(got, d, "stream, hits=%s" % hits)
        for x, y in zip(got, one_shot):
            assert x.tobytes() == y.tobytes()
        tots.append(tot)
    assert tots[0] == tots[1] == gr.counters


def test_merge_eq_classes_without_a_process_group(small, small_default):
    """dist.merge_eq_classes with no process group: the table comes back as it is, as all_reduce_counters does for counters"""
    import rapmap_amd as ra
    from rapmap_amd import dist
    gr, d, one_shot = small_default
    t = ra.EqClasses(small["mp"])
    t.add_labels(*one_shot)
    assert dist.merge_eq_classes(t, small["mp"]) is t
    for x, y in zip(t.fetch(), one_shot):
        assert x.tobytes() == y.tobytes()
    assert t.stat(t.LAST_FOLD_US) > 0
    t.close()


def test_stream_flags_are_checked(small, small_fastq):
    import rapmap_amd as ra
    with pytest.raises(ValueError):
        ra.MappedStream(small["qi"], small_fastq[0], small_fastq[1], hits=False)
    st = ra.MappedStream(small["qi"], small_fastq[0], small_fastq[1], batch_units=2000, threads=2)
    with pytest.raises(ra.QmError):
        st.eq_classes()                                           # opened without eq_classes
    st.close()


@pytest.mark.parametrize("no_output", [False, True])
def test_cli_eq_classes(sample_data, tmp_path, no_output):
    import rapmap_amd as ra
    sd = os.path.join(GOLD, "sample_data")
    eq = str(tmp_path / "eq_classes.txt")
    args = ["quasimap", "-i", sample_data["idx"], "-1", os.path.join(sd, "reads_1.fastq.gz"), "-2", os.path.join(sd, "reads_2.fastq.gz"),
            "--eqClasses", eq, "-t", "4", "-q"] + (["-n"] if no_output else ["-o", str(tmp_path / "out.sam")])
    r = subprocess.run([sys.executable, "-m", "rapmap_amd"] + args, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    qi = ra.QuasiIndex(sample_data["idx"])
    mp = ra.QuasiMapper(qi, 0)
    q1, o1 = pack(sample_data["reads1"]); q2, o2 = pack(sample_data["reads2"])
    gr = mp.map_pairs(q1, o1, q2, o2)
    names, off, tids, cnt = ra.read_eq_classes(eq)
    assert names == qi.txp_names
    ec.assert_table((off, tids, cnt), ec.expected_from_hits(gr.hit_offsets, gr.hits), "--eqClasses" + (" -n" if no_output else ""))
    mp.close()
