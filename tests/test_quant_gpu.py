"""Abundance estimation on the device (qm_quant_*, Quant, EqClasses.quantify, quasimap --quant) against the numpy restatement of the
model in quant_cases.py.  Tables are filled through add_labels, so most tests need no mapping at all; the synth_small table is the
one the device builds from its own mapping.  The checks are quant_cases.py's, the same the lane emulation runs (test_quant.py).
Run on the MI355X box: -m gpu.

The ABI takes the table alone (qm_quant_create(qm_eqc*, ...)): a quant object lives on its table's device and runs on a stream of its
own, so there is no second context whose device could differ from the table's.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import eqc_cases as ec
import quant_cases as qc
from conftest import GOLD, ROOT
from util import pack

pytestmark = pytest.mark.gpu


class ArgError(Exception):
    """QM_E_ARG"""


def make_solver(mp, table=None):
    """quant_cases' solve() on the device: the canonical arrays folded into a fresh table (or `table` as it is), then Quant"""
    import rapmap_amd as ra

    def f(off, tids, cnt, n_txps, eff=None, alpha0=None, **kw):
        t = table
        if t is None:
            t = ra.EqClasses(mp, expected=64)
            if len(off) > 1:
                t.add_labels(off, tids, cnt)
        q = None
        try:
            q = ra.Quant(t, n_txps, eff)
            if alpha0 is not None:
                q.set_start(alpha0)
            it, rel = q.run(**kw)
            st = q.stat(); st["iterations"] = it
            assert st["last_run_us"] > 0 or it == 0
            return q.fetch(), it, rel, st
        except ra.QmError as e:
            if "error -1:" in str(e):
                raise ArgError(str(e))
            raise
        finally:
            if q is not None:
                q.close()
            if table is None:
                t.close()
    return f


@pytest.fixture(scope="module")
def small(synth_small):
    import rapmap_amd as ra
    qi = ra.QuasiIndex(synth_small["idx"])
    mp = ra.QuasiMapper(qi, 0, debug=False)
    q1, o1 = pack(synth_small["reads1"]); q2, o2 = pack(synth_small["reads2"])
    yield {"qi": qi, "mp": mp, "q1": q1, "o1": o1, "q2": q2, "o2": o2}
    mp.close()


@pytest.fixture(scope="module")
def solve(small):
    return make_solver(small["mp"])


@pytest.fixture(scope="module")
def crafted(solve):
    L, w, nt, eff = qc.crafted_table()
    return qc.Graph(*qc.table_of(L, w), nt), eff, solve


@pytest.fixture(scope="module")
def small_table(small):
    """the default mapping of synth_small folded on the device: the table (never changed), its graph, random effective lengths,
    and a solver that runs on that very table"""
    import rapmap_amd as ra
    mp = small["mp"]
    mp.map_pairs(small["q1"], small["o1"], small["q2"], small["o2"])
    t = ra.EqClasses(mp)
    t.add(mp)
    nt = small["qi"].n_txps
    yield qc.Graph(*t.fetch(), nt), qc.random_eff(nt), make_solver(mp, t)
    t.close()


@pytest.fixture(scope="module", params=["crafted", "synth_small"])
def table(request):
    return request.param, request.getfixturevalue("crafted" if request.param == "crafted" else "small_table")


def test_one_step_bit_exact(solve):
    qc.check_one_step(solve)


def test_fixed_point(solve):
    qc.check_fixed_point(solve)


def test_against_restatement(table):
    name, (g, eff, solve) = table
    qc.check_against_restatement(solve, g, eff, name)


def test_invariants(table):
    name, (g, eff, solve) = table
    qc.check_invariants(solve, g, eff, name)


def test_single_tid_classes(table):
    """exact equality.  The device code takes single-tid classes out of the sums and adds their count as it is; the numpy restatement,
    which multiplies w_t by n_c / w_t, ends one unit in the last place off for 10 of synth_small's 132 such transcripts (1.27e-16).
    The crafted table has no such transcript."""
    name, (g, eff, solve) = table
    qc.check_single_tid_classes(solve, g, eff, name)


def test_stopping_rule(small_table):
    g, eff, solve = small_table
    qc.check_stopping_rule(solve, g, eff, "synth_small")


def test_determinism_and_snapshot(small, crafted):
    import rapmap_amd as ra
    g, eff, _ = crafted
    t = ra.EqClasses(small["mp"], expected=64)
    t.add_labels(g.off, g.tid, g.cnt)
    q = ra.Quant(t, g.nt, eff)
    assert q.run(max_iter=30, rel_tol=0.0) == (30, -1.0)
    a = q.fetch()
    q.set_start(None)
    q.run(max_iter=30, rel_tol=0.0)
    assert q.fetch().tobytes() == a.tobytes()                       # two runs from the same start on one object
    p = ra.Quant(t, g.nt, eff)
    p.run(max_iter=30, rel_tol=0.0)
    assert p.fetch().tobytes() == a.tobytes()                       # a second object on the same table
    p.set_start(None)
    p.run(max_iter=12, rel_tol=0.0); p.run(max_iter=18, rel_tol=0.0)
    assert p.fetch().tobytes() == a.tobytes()                       # a run goes on where the last one stopped
    before = q.stat()
    t.add_labels(*ec.csr(ec.distinct_labels(5000)))                 # the table grows and is rebuilt: nothing of it is where it was
    q.set_start(None)
    q.run(max_iter=30, rel_tol=0.0)
    assert q.fetch().tobytes() == a.tobytes()
    after = q.stat()
    assert {k: v for k, v in after.items() if k != "last_run_us"} == {k: v for k, v in before.items() if k != "last_run_us"}
    t.close()                                                       # ... and the object outlives its table
    q.set_start(None)
    q.run(max_iter=30, rel_tol=0.0)
    assert q.fetch().tobytes() == a.tobytes()
    p.close(); q.close()


def test_errors_and_edges(solve):
    qc.check_errors_and_edges(solve, ArgError)


def test_run_arguments_are_checked(small):
    import rapmap_amd as ra
    t = ra.EqClasses(small["mp"], expected=16)
    t.add_labels([0, 2, 3], [0, 1, 1])
    q = ra.Quant(t, 2)
    for kw in (dict(max_iter=-1), dict(check_every=0), dict(rel_tol=-1.0), dict(rel_tol=float("nan")), dict(min_alpha=-1.0)):
        with pytest.raises(ra.QmError, match="-1"):
            q.run(**kw)
    with pytest.raises(ValueError):
        ra.Quant(t, 2, [1.0, 2.0, 3.0])
    g = qc.Graph(*t.fetch(), 2)
    qc.assert_close(t.quantify(2, max_iter=3, rel_tol=0.0), qc.iterate(g, np.ones(2), g.uniform_start(), 3), "quantify, 3 iterations")
    q.close(); t.close()


@pytest.fixture(scope="module")
def small_fastq(synth_small, tmp_path_factory):
    d = tmp_path_factory.mktemp("quant_fq")
    f1, f2 = str(d / "r1.fastq"), str(d / "r2.fastq")
    for fn, nms, rds in ((f1, synth_small["names1"], synth_small["reads1"]), (f2, synth_small["names2"], synth_small["reads2"])):
        with open(fn, "wb") as fh:
            for nm, r in zip(nms, rds):
                fh.write(b"@" + nm.encode() + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
    return f1, f2


def test_stream_to_abundances(small, small_table, small_fastq):
    """FASTQ -> classes -> abundances with no hit on the host: the stream's merged table gives what the one-shot table gives"""
    import rapmap_amd as ra
    g, eff, solve = small_table
    st = ra.MappedStream(small["qi"], small_fastq[0], small_fastq[1], batch_units=500, threads=3, names=False, eq_classes=True, hits=False)
    for b in st:
        assert b.hits is None
    got = st.eq_classes()
    st.close()
    t = ra.EqClasses(small["mp"])
    t.add_labels(*got)
    a = t.quantify(g.nt, eff, max_iter=25, rel_tol=0.0)
    t.close()
    qc.assert_close(a, qc.iterate(g, eff, g.uniform_start(), 25), "stream, 25 iterations")


def _cli(args):
    r = subprocess.run([sys.executable, "-m", "rapmap_amd", "quasimap"] + args, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r


def _sample_args(sample_data):
    sd = os.path.join(GOLD, "sample_data")
    return ["-i", sample_data["idx"], "-1", os.path.join(sd, "reads_1.fastq.gz"), "-2", os.path.join(sd, "reads_2.fastq.gz"), "-t", "4", "-n"]


def test_cli_quant(sample_data, tmp_path):
    import rapmap_amd as ra
    qf = str(tmp_path / "q.sf")
    r = _cli(_sample_args(sample_data) + ["--quant", qf])
    assert "EM iterations" in r.stderr
    qi = ra.QuasiIndex(sample_data["idx"])
    mp = ra.QuasiMapper(qi, 0)
    q1, o1 = pack(sample_data["reads1"]); q2, o2 = pack(sample_data["reads2"])
    mp.map_pairs(q1, o1, q2, o2)
    t = ra.EqClasses(mp); t.add(mp)
    lens = np.asarray(qi.txp_lens, dtype=np.float64)
    alpha = t.quantify(qi.n_txps, lens)
    names, l2, e2, tpm, reads = ra.read_quant(qf)
    assert names == qi.txp_names and np.array_equal(l2, qi.txp_lens) and np.array_equal(e2, lens)
    qc.assert_close(reads, alpha, "--quant against EqClasses.quantify")
    assert abs(float(tpm.sum()) - 1e6) <= 1e-6
    t.close(); mp.close()


def test_cli_quant_with_eq_classes(sample_data, tmp_path):
    import rapmap_amd as ra
    qf, e1, e2 = str(tmp_path / "q.sf"), str(tmp_path / "eq_with.txt"), str(tmp_path / "eq_without.txt")
    _cli(_sample_args(sample_data) + ["-q", "--quant", qf, "--eqClasses", e1, "--quantFragLenMean", "100.5", "--quantMaxIter", "40", "--quantRelTol", "0"])
    _cli(_sample_args(sample_data) + ["-q", "--eqClasses", e2])
    assert open(e1, "rb").read() == open(e2, "rb").read()
    names, lens, eff, tpm, reads = ra.read_quant(qf)
    assert np.array_equal(eff, np.maximum(1.0, lens - 100.5 + 1))
    n2, off, tids, cnt = ra.read_eq_classes(e1)
    g = qc.Graph(off, tids, cnt, len(names))
    qc.assert_close(reads, qc.iterate(g, eff, g.uniform_start(), 40), "--quant --eqClasses, 40 iterations")
    assert abs(float(tpm.sum()) - 1e6) <= 1e-6
