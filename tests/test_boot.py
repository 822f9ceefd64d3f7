"""Bootstrap replicates without a GPU: the device code (rapmap_amd/csrc/qm_boot.inl) under the lane emulation, the restatement of the
draw, the file format, the CLI's argument check.

The emulation (tests/emu/qm_emu_boot.cpp) runs one wavefront after the other and one lane after the other: it proves the draw, the
logic of the batched iteration bodies, the fixed order of their sums and the per-replicate stop -- not the atomics or the launches,
which are the GPU tests' part (test_boot_gpu.py).  Both files run the checks of boot_cases.py; here the synth_small table comes from
the oracle's hits instead of the device's."""
import subprocess
import sys

import numpy as np
import pytest

import boot_cases as bc
import eqc_cases as ec
import quant_cases as qc
from conftest import ROOT, load_oracle
from util import pack


@pytest.fixture(scope="module")
def env():
    import emu_boot
    import emu_quant
    emu_boot._lib(); emu_quant._lib()

    class Env:
        ArgError, StateError = emu_boot.ArgError, emu_boot.StateError
        make = staticmethod(lambda off, tids, cnt, n_txps, eff, n_reps: emu_boot.Boot(off, tids, cnt, n_txps, eff, n_reps))
        solve = staticmethod(emu_quant.run)
    return Env


@pytest.fixture(scope="module")
def crafted():
    return bc.crafted_graph()


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


def test_philox_known_answers():
    import emu_boot
    bc.check_philox_restatement()
    for ctr, key, out in bc.PHILOX_ANSWERS:                           # ... and the device's own function, as the emulation compiles it
        assert tuple(int(x) for x in emu_boot.philox(ctr, key)) == out


def test_emulated_draws_exact(env):
    bc.check_draws_exact(env)


def test_emulated_aggregation_gives_the_same_counts():
    """the resample's per-wavefront aggregation is a way to issue fewer atomics, not another draw"""
    import emu_boot
    L, n, nt = bc.seven_class_table()
    off, tids, cnt = qc.table_of(L, n)
    a, b = emu_boot.Boot(off, tids, cnt, nt, None, 3, aggregate=0), emu_boot.Boot(off, tids, cnt, nt, None, 3, aggregate=1)
    a.resample(seed=5, first_rep=2); b.resample(seed=5, first_rep=2)
    for rep in range(3):
        assert np.array_equal(a.counts(rep), b.counts(rep)) and np.array_equal(a.counts(rep), bc.draw_counts(a.classes()[2], 5, 2 + rep))
    a.close(); b.close()


def test_emulated_slots_do_not_matter(env):
    bc.check_slots_do_not_matter(env)


def test_emulated_one_step_bit_exact(env):
    bc.check_one_step(env)


def test_emulated_fixed_point(env):
    bc.check_fixed_point(env)


def test_emulated_against_restatement_and_quant(env, table):
    name, (g, eff) = table
    alone = bc.check_against_restatement(env, g, eff, name)
    assert alone > 0 or name == "crafted"                            # (the crafted table has no transcript of single-tid classes only)


def test_emulated_invariants(env, table):
    name, (g, eff) = table
    bc.check_invariants(env, g, eff, name)


def test_emulated_zero_count_class(env):
    bc.check_zero_count_class(env)


def test_the_scheme(env):
    """64 replicates of the seven-class table under seed 12345: by the restatement alone (at most 1.33 standard errors off), then by the
    emulation (whose snapshot order is another one)"""
    L, n, nt = bc.seven_class_table()
    z = bc.scheme_statistics(lambda r: bc.draw_counts(n, 12345, r), n)
    assert z <= 1.34
    off, tids, cnt = qc.table_of(L, n)
    b = env.make(off, tids, cnt, nt, None, 64)
    b.resample(seed=12345)
    bc.scheme_statistics(lambda r: b.counts(r), b.classes()[2])
    b.close()


def test_emulated_errors(env):
    bc.check_errors(env)


def test_emulated_lifetime(env):
    """what test_boot_gpu.py's test_lifetime_and_snapshot asks of the device objects, of the emulated ones: closing a quant object that a
    boot object borrows is refused and destroys nothing, a run goes on where the last one stopped, the launches are counted"""
    import emu_boot
    import emu_quant
    L, n, nt = bc.mixed_table()
    off, tids, cnt = qc.table_of(L, n)
    q = emu_quant.Quant(off, tids, cnt, nt, lib=emu_boot._lib())
    b = emu_boot.Boot(None, None, None, nt, None, 4, quant=q)
    with pytest.raises(env.StateError):
        q.close()
    b.resample(seed=3)
    before = [b.counts(r) for r in range(4)]
    b.run(max_iter=12, rel_tol=0.0)
    a = b.fetch()
    assert b.launches == 24 and b.info["draws"] == int(cnt.sum())
    assert q.run(max_iter=3, rel_tol=0.0) == (3, -1.0)                # the quant object is still whole
    b.resample(seed=3)
    assert all(np.array_equal(b.counts(r), before[r]) for r in range(4))
    b.run(max_iter=5, rel_tol=0.0); b.run(max_iter=7, rel_tol=0.0)     # a run goes on where the last one stopped
    assert b.fetch().tobytes() == a.tobytes()
    with pytest.raises(env.StateError):
        q.close()
    b.close()
    q.close()


def test_emulated_determinism(env):
    bc.check_determinism(env)


def test_tolerance_record_matches_the_constant(env, crafted, small):
    """the measurement behind boot_cases.REL_TOL, taken again on replicate tables (the restatement's draws, seed 7, 17 replicates)"""
    worst = 0.0
    for name, (g, eff) in (("crafted", crafted), ("synth_small", small)):
        reps = {"%s/%d" % (name, r): (qc.Graph(g.off, g.tid, bc.draw_counts(g.cnt, 7, r), g.nt), eff) for r in range(17)}
        m = qc.measure_tolerance(reps)
        worst = max(worst, max(v for r in m.values() for v in r.values()))
    print("largest CPU-to-CPU difference over the replicate tables: %.3g" % worst)
    assert bc.MEASURED_MAX_REL_REPLICATES * 0.9 <= worst <= bc.MEASURED_MAX_REL_REPLICATES * 1.1
    assert bc.REL_TOL == max(qc.REL_TOL, 64 * bc.MEASURED_MAX_REL_REPLICATES)


def test_write_read_bootstraps_round_trip(tmp_path):
    import rapmap_amd as ra
    rng = np.random.default_rng(2)
    a = rng.random((3, 7)) * 1e6
    a[1, 2] = 0.0; a[2, 6] = 5e-324
    p = str(tmp_path / "q.sf.bootstraps.gz")
    ra.write_bootstraps(p, a)
    import gzip
    raw = gzip.open(p, "rb").read()
    assert raw == a.astype("<f8").tobytes()                          # B x n_txps little-endian float64, row-major
    assert ra.read_bootstraps(p, 7).tobytes() == a.tobytes() and ra.read_bootstraps(p, 7).shape == (3, 7)
    with pytest.raises(ValueError):
        ra.read_bootstraps(p, 4)                                     # 21 numbers are no whole number of rows of 4


def test_cli_rejects_bootstraps_without_quant():
    r = subprocess.run([sys.executable, "-m", "rapmap_amd", "quasimap", "-i", "nowhere", "-r", "reads.fq", "--numBootstraps", "3"],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 2 and "--numBootstraps needs --quant" in r.stderr
