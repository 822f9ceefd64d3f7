"""Abundance estimation without a GPU: the device code (rapmap_amd/csrc/qm_quant.inl) under the lane emulation, the file format, the CLI.

The emulation (tests/emu/qm_emu_quant.cpp) runs one wavefront after the other and one lane after the other, with host-side scans and a
stable sort standing in for rocPRIM: it proves the LOGIC of the structure build and of the two iteration bodies, and the fixed order of
their sums -- not the atomics or the launches, which are the GPU tests' part (test_quant_gpu.py).  Both files run the checks of
quant_cases.py; here the synth_small table comes from the oracle's hits instead of the device's."""
import subprocess
import sys

import numpy as np
import pytest

import eqc_cases as ec
import quant_cases as qc
from conftest import ROOT, load_oracle
from util import pack


@pytest.fixture(scope="module")
def solve():
    import emu_quant
    emu_quant._lib()

    def f(off, tids, cnt, n_txps, eff=None, alpha0=None, **kw):
        return emu_quant.run(off, tids, cnt, n_txps, eff, alpha0, **kw)
    return f


@pytest.fixture(scope="module")
def crafted():
    L, w, nt, eff = qc.crafted_table()
    return qc.Graph(*qc.table_of(L, w), nt), eff


@pytest.fixture(scope="module")
def small(synth_small, oracle_mod):
    """the table of synth_small under default options, from the oracle's hits; random effective lengths"""
    ix, orc = load_oracle(synth_small["idx"])
    q1, o1 = pack(synth_small["reads1"]); q2, o2 = pack(synth_small["reads2"])
    res = orc.map_pairs(q1, o1, q2, o2, nthreads=4)
    nt = len(ix.names)
    return qc.Graph(*ec.canonical(ec.expected_from_hits(res.hit_offsets, res.hits)), nt), qc.random_eff(nt)


@pytest.fixture(scope="module", params=["crafted", "synth_small"])
def table(request):
    return request.param, request.getfixturevalue("crafted" if request.param == "crafted" else "small")


def test_emulated_one_step_bit_exact(solve):
    qc.check_one_step(solve)


def test_emulated_fixed_point(solve):
    qc.check_fixed_point(solve)


def test_emulated_against_restatement(solve, table):
    name, (g, eff) = table
    qc.check_against_restatement(solve, g, eff, name)


def test_emulated_invariants(solve, table):
    name, (g, eff) = table
    qc.check_invariants(solve, g, eff, name)


def test_emulated_single_tid_classes(solve, table):
    """exact equality.  The device code takes single-tid classes out of the sums and adds their count as it is; the numpy restatement,
    which multiplies w_t by n_c / w_t, ends one unit in the last place off for 10 of synth_small's 132 such transcripts (1.27e-16).
    The crafted table has no such transcript."""
    name, (g, eff) = table
    qc.check_single_tid_classes(solve, g, eff, name)


def test_emulated_stopping_rule(solve, small):
    g, eff = small
    qc.check_stopping_rule(solve, g, eff, "synth_small")


def test_emulated_determinism_and_continuation(solve, crafted):
    g, eff = crafted
    a = solve(g.off, g.tid, g.cnt, g.nt, eff, None, max_iter=7, rel_tol=0.0)[0]
    b = solve(g.off, g.tid, g.cnt, g.nt, eff, None, max_iter=7, rel_tol=0.0)[0]
    assert a.tobytes() == b.tobytes()
    c = solve(g.off, g.tid, g.cnt, g.nt, eff, None, max_iter=4, rel_tol=0.0)[0]
    c = solve(g.off, g.tid, g.cnt, g.nt, eff, c, max_iter=3, rel_tol=0.0)[0]          # 4 + 3 iterations: a run goes on where the last one stopped
    assert a.tobytes() == c.tobytes()


def test_emulated_object_runs_again(solve, crafted):
    """what test_quant_gpu.py asks of one object on the device, of the emulated one: a run from the same start repeats bit for bit, a
    second object on the same table agrees, a run goes on where the last one stopped, and the statistics stay"""
    import emu_quant
    g, eff = crafted
    q = emu_quant.Quant(g.off, g.tid, g.cnt, g.nt, eff)
    assert q.run(max_iter=30, rel_tol=0.0) == (30, -1.0)
    a = q.fetch(); before = q.stat()
    q.set_start(None)
    q.run(max_iter=30, rel_tol=0.0)
    assert q.fetch().tobytes() == a.tobytes()
    p = emu_quant.Quant(g.off, g.tid, g.cnt, g.nt, eff)
    p.run(max_iter=12, rel_tol=0.0); p.run(max_iter=18, rel_tol=0.0)
    assert p.fetch().tobytes() == a.tobytes() and q.stat() == before == p.stat()
    for kw in (dict(max_iter=-1), dict(check_every=0), dict(rel_tol=-1.0), dict(rel_tol=float("nan")), dict(min_alpha=-1.0)):
        with pytest.raises(emu_quant.ArgError):
            q.run(**kw)
    p.close(); q.close()


def test_emulated_errors_and_edges(solve):
    import emu_quant
    qc.check_errors_and_edges(solve, emu_quant.ArgError)


def test_tolerance_record_matches_the_constant(crafted, small):
    """the measurement behind quant_cases.REL_TOL, taken again: the recorded maximum is what these inputs give (to the digits kept)"""
    m = qc.measure_tolerance({"crafted": crafted, "synth_small": small})
    worst = max(v for r in m.values() for v in r.values())
    print(m)
    assert qc.MEASURED_MAX_REL * 0.9 <= worst <= qc.MEASURED_MAX_REL * 1.1
    assert qc.REL_TOL == max(1e-13, 64 * qc.MEASURED_MAX_REL)


def test_write_read_quant_round_trip(tmp_path):
    import rapmap_amd as ra
    rng = np.random.default_rng(1)
    names = ["t%d" % i for i in range(6)] + ["a name|with.odd:chars"]
    lens = np.array([100, 2000, 31, 50000, 7, 1, 12345], dtype=np.int64)
    eff = np.maximum(1.0, lens - 180.5 + 1)
    alpha = np.array([0.0, 1.0 / 3.0, 1e-300, 123456789.12345678, 5e-324, 2.0 ** 52 + 1, rng.random()])
    p = str(tmp_path / "quant.sf")
    ra.write_quant(p, names, lens, eff, alpha)
    lines = open(p).read().split("\n")
    assert lines[0] == "Name\tLength\tEffectiveLength\tTPM\tNumReads" and len(lines) == 9 and lines[-1] == ""
    assert lines[1].split("\t")[:3] == ["t0", "100", "1.0"] and lines[1].split("\t")[4] == "0.0"
    n2, l2, e2, tpm, a2 = ra.read_quant(p)
    assert n2 == names and np.array_equal(l2, lens) and np.array_equal(e2, eff)
    assert a2.tobytes() == alpha.tobytes()                           # NumReads comes back bit for bit
    rate = alpha / eff
    assert np.array_equal(tpm, rate / rate.sum() * 1e6) and abs(tpm.sum() - 1e6) <= 1e-6
    with pytest.raises(ValueError):
        ra.write_quant(p, names[:3], lens, eff, alpha)


def test_cli_rejects_quant_without_a_file():
    r = subprocess.run([sys.executable, "-m", "rapmap_amd", "quasimap", "-i", "nowhere", "-r", "reads.fq", "--quant"],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 2 and "--quant" in r.stderr and "expected one argument" in r.stderr
