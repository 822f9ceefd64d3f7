"""Bootstrap replicates on the device (qm_boot_*, Bootstrap, Quant.bootstrap, quasimap --numBootstraps) against the numpy restatement of
the draw and of the model (boot_cases.py, quant_cases.py).  Tables are filled through add_labels, so most tests need no mapping at
all; the synth_small table is the one the device builds from its own mapping.  The checks are boot_cases.py's, the same the lane
emulation runs (test_boot.py).  Run on the MI355X box: -m gpu."""
import os
import subprocess
import sys

import numpy as np
import pytest

import boot_cases as bc
import eqc_cases as ec
import quant_cases as qc
from conftest import ROOT
from util import pack

pytestmark = pytest.mark.gpu


class ArgError(Exception):
    """QM_E_ARG"""


class StateError(Exception):
    """QM_E_STATE"""


def _translate(e):
    if "error -1:" in str(e):
        return ArgError(str(e))
    if "error -7:" in str(e):
        return StateError(str(e))
    return e


class DeviceBoot:
    """what boot_cases' env.make returns: a table (filled through add_labels unless given), its Quant and a Bootstrap of it"""

    def __init__(self, mp, off, tids, cnt, n_txps, eff, n_reps, table=None):
        import rapmap_amd as ra
        self.n_txps, self.n_reps = int(n_txps), int(n_reps)
        self.own = table is None
        self.t = table if table is not None else ra.EqClasses(mp, expected=64)
        self.q = self.b = None
        try:
            if self.own and len(off) > 1:
                self.t.add_labels(off, tids, cnt)
            self.q = ra.Quant(self.t, n_txps, eff)
            self.b = ra.Bootstrap(self.q, n_reps)
        except ra.QmError as e:
            self.close()
            raise _translate(e)

    def classes(self):
        return self.q.classes()

    def resample(self, seed=0, first_rep=0):
        self.b.resample(seed=seed, first_rep=first_rep)

    def _call(self, f, *a, **kw):
        import rapmap_amd as ra
        try:
            return f(*a, **kw)
        except ra.QmError as e:
            raise _translate(e)

    def set_counts(self, rep, counts):
        self._call(self.b.set_counts, rep, counts)

    def counts(self, rep):
        return self._call(self.b.counts, rep)

    def run(self, **kw):
        return self._call(self.b.run, **kw)

    def fetch(self):
        return self.b.fetch()

    def close(self):
        if self.b is not None:
            self.b.close()
        if self.q is not None:
            self.q.close()
        if self.own:
            self.t.close()
        self.b = self.q = None


@pytest.fixture(scope="module")
def small(synth_small):
    import rapmap_amd as ra
    qi = ra.QuasiIndex(synth_small["idx"])
    mp = ra.QuasiMapper(qi, 0, debug=False)
    q1, o1 = pack(synth_small["reads1"]); q2, o2 = pack(synth_small["reads2"])
    yield {"qi": qi, "mp": mp, "q1": q1, "o1": o1, "q2": q2, "o2": o2}
    mp.close()


def make_solver(mp, table=None):
    """quant_cases' solve() on the device: the canonical arrays folded into a fresh table (or `table` as it is), then Quant"""
    import rapmap_amd as ra

    def f(off, tids, cnt, n_txps, eff=None, alpha0=None, **kw):
        t = table
        if t is None:
            t = ra.EqClasses(mp, expected=64)
            if len(off) > 1:
                t.add_labels(off, tids, cnt)
        q = ra.Quant(t, n_txps, eff)
        try:
            if alpha0 is not None:
                q.set_start(alpha0)
            it, rel = q.run(**kw)
            return q.fetch(), it, rel, q.stat()
        finally:
            q.close()
            if table is None:
                t.close()
    return f


def make_env(mp, table=None):
    class Env:
        pass
    Env.ArgError, Env.StateError = ArgError, StateError
    # one table per input, shared by every object made from that input: a draw is defined against the snapshot's order, and two
    # tables filled with the same labels need not lay them out alike once they have grown (which claim is published before a
    # table fills up is a race), so "the same replicate" means the same table
    Env.tables = {}

    def make(off, tids, cnt, n_txps, eff, n_reps):
        import rapmap_amd as ra
        t = table
        if t is None:
            off, tids, cnt = np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(tids, dtype=np.uint32), np.ascontiguousarray(cnt, dtype=np.uint64)
            key = (off.tobytes(), tids.tobytes(), cnt.tobytes())
            if key not in Env.tables:
                Env.tables[key] = ra.EqClasses(mp, expected=64)
                if len(off) > 1:
                    Env.tables[key].add_labels(off, tids, cnt)
            t = Env.tables[key]
        return DeviceBoot(mp, off, tids, cnt, n_txps, eff, n_reps, t)
    Env.make = staticmethod(make)
    Env.solve = staticmethod(make_solver(mp, table))
    return Env


@pytest.fixture(scope="module")
def env(small):
    e = make_env(small["mp"])
    yield e
    for t in e.tables.values():
        t.close()


@pytest.fixture(scope="module")
def crafted(env):
    return bc.crafted_graph() + (env,)


@pytest.fixture(scope="module")
def small_table(small):
    """the default mapping of synth_small folded on the device: its graph, random effective lengths, and an env whose objects are made
    on that very table (never changed)"""
    import rapmap_amd as ra
    mp = small["mp"]
    mp.map_pairs(small["q1"], small["o1"], small["q2"], small["o2"])
    t = ra.EqClasses(mp)
    t.add(mp)
    nt = small["qi"].n_txps
    yield qc.Graph(*t.fetch(), nt), qc.random_eff(nt), make_env(mp, t)
    t.close()


@pytest.fixture(scope="module", params=["crafted", "synth_small"])
def table(request):
    return request.param, request.getfixturevalue("crafted" if request.param == "crafted" else "small_table")


def test_philox_known_answers(env):
    """the restatement's known answers; the device's generator through a table of two classes of one fragment each: N = 2, so draw 0 falls
    into class (top bit of x1) and draw 1 into class (top bit of x3) of Philox(0, 0, lo R, hi R; seed) -- for R = 0 and seed 0 that is the
    first known answer, whose x1 = e169c58d and x3 = 9b00dbd8 both have the top bit set"""
    bc.check_philox_restatement()
    off, tids, cnt = qc.table_of([[0], [1]], np.array([1, 1], dtype=np.uint64))
    b = env.make(off, tids, cnt, 2, None, 3)
    for seed in (0, 0x299f31d0a4093822):
        b.resample(seed=seed, first_rep=0)
        for rep in range(3):
            x = bc.philox(0, 0, rep, 0, seed & 0xffffffff, seed >> 32)
            want = np.bincount([int(x[1][0]) >> 31, int(x[3][0]) >> 31], minlength=2)
            assert b.counts(rep).tolist() == want.tolist(), (seed, rep)
    b.resample(seed=0, first_rep=0)
    assert b.counts(0).tolist() == [0, 2]
    b.close()


def test_draws_exact(env):
    bc.check_draws_exact(env)


def test_slots_do_not_matter(env):
    bc.check_slots_do_not_matter(env)


def test_one_step_bit_exact(env):
    bc.check_one_step(env)


def test_fixed_point(env):
    bc.check_fixed_point(env)


def test_against_restatement_and_quant(table):
    name, (g, eff, env) = table
    alone = bc.check_against_restatement(env, g, eff, name)
    assert alone > 0 or name == "crafted"


def test_invariants(table):
    name, (g, eff, env) = table
    bc.check_invariants(env, g, eff, name)


def test_zero_count_class(env):
    bc.check_zero_count_class(env)


def test_errors(env):
    bc.check_errors(env)


def test_determinism(env):
    bc.check_determinism(env)


def test_lifetime_and_snapshot(small):
    """Quant.close() with a live Bootstrap raises and destroys nothing; folding into or clearing the table afterwards changes nothing"""
    import rapmap_amd as ra
    L, n, nt = bc.mixed_table()
    off, tids, cnt = qc.table_of(L, n)
    t = ra.EqClasses(small["mp"], expected=64)
    t.add_labels(off, tids, cnt)
    q = ra.Quant(t, nt)
    b = ra.Bootstrap(q, 4)
    with pytest.raises(ra.QmError, match="-7"):
        q.close()
    b.resample(seed=3)
    before = (q.classes(), [b.counts(r) for r in range(4)])
    b.run(max_iter=12, rel_tol=0.0)
    a = b.fetch()
    st = b.stat()
    assert (st["replicates"], st["draws"], st["launches"]) == (4, int(cnt.sum()), 24) and st["last_run_us"] > 0 and st["last_resample_us"] > 0
    assert q.run(max_iter=3, rel_tol=0.0) == (3, -1.0)                # the quant object is still whole
    t.add_labels(*ec.csr(ec.distinct_labels(5000)))                 # the table grows and is rebuilt: nothing of it is where it was
    t.clear()
    b.resample(seed=3)
    assert all(np.array_equal(x, y) for x, y in zip(before[0], q.classes())) and all(np.array_equal(b.counts(r), before[1][r]) for r in range(4))
    b.run(max_iter=12, rel_tol=0.0)
    assert b.fetch().tobytes() == a.tobytes()
    t.close()                                                       # ... and both outlive the table
    b.resample(seed=3); b.run(max_iter=5, rel_tol=0.0); b.run(max_iter=7, rel_tol=0.0)     # a run goes on where the last one stopped
    assert b.fetch().tobytes() == a.tobytes()
    assert q.bootstrap(4, seed=3, max_iter=12, rel_tol=0.0).tobytes() == a.tobytes()       # the one-call form
    with pytest.raises(ra.QmError, match="-7"):
        q.close()
    b.close()
    q.close()


def test_aggregated_resample_gives_the_same_counts(small):
    """QM_BOOT_AGGREGATE=1 (the variant measured in DESIGN.md section 4.11 (a)) is a way to issue fewer atomics, not another draw"""
    import rapmap_amd as ra
    L, n, nt = bc.seven_class_table()
    off, tids, cnt = qc.table_of(L, n)
    t = ra.EqClasses(small["mp"], expected=64)
    t.add_labels(off, tids, cnt)
    q = ra.Quant(t, nt)
    got = []
    for flag in ("0", "1"):
        os.environ["QM_BOOT_AGGREGATE"] = flag
        try:
            b = ra.Bootstrap(q, 2)
        finally:
            del os.environ["QM_BOOT_AGGREGATE"]
        b.resample(seed=12345, first_rep=5)
        got.append([b.counts(r) for r in range(2)])
        b.close()
    scnt = q.classes()[2]
    for r in range(2):
        assert np.array_equal(got[0][r], got[1][r]) and np.array_equal(got[0][r], bc.draw_counts(scnt, 12345, 5 + r))
    q.close(); t.close()


@pytest.fixture(scope="module")
def small_fastq(synth_small, tmp_path_factory):
    d = tmp_path_factory.mktemp("boot_fq")
    f1, f2 = str(d / "r1.fastq"), str(d / "r2.fastq")
    for fn, nms, rds in ((f1, synth_small["names1"], synth_small["reads1"]), (f2, synth_small["names2"], synth_small["reads2"])):
        with open(fn, "wb") as fh:
            for nm, r in zip(nms, rds):
                fh.write(b"@" + nm.encode() + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
    return f1, f2


def test_cli_bootstraps(synth_small, small, small_table, small_fastq, tmp_path):
    import rapmap_amd as ra
    g, _, env = small_table
    qf = str(tmp_path / "q.sf")
    args = [sys.executable, "-m", "rapmap_amd", "quasimap", "-i", synth_small["idx"], "-1", small_fastq[0], "-2", small_fastq[1], "-t", "4", "-n", "-q"]
    r = subprocess.run(args + ["--quant", qf, "--numBootstraps", "3", "--bootstrapSeed", "7"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    nt = small["qi"].n_txps
    names, lens, eff, tpm, reads = ra.read_quant(qf)
    got = ra.read_bootstraps(qf + ".bootstraps.gz", nt)
    assert got.shape == (3, nt)
    # by hand, on a table filled the way the CLI fills its own (a table of the default size, the stream's sorted classes in one
    # add_labels: the claim of a slot goes to the lowest unit index, so equal input gives equal slots, hence the same snapshot order)
    t = ra.EqClasses(small["mp"])
    t.add_labels(g.off, g.tid, g.cnt)
    q = ra.Quant(t, nt, eff)
    for i in range(3):                                               # row i: replicate number i, whatever batch or slot it ran in
        b = ra.Bootstrap(q, 1)
        b.resample(seed=7, first_rep=i)
        b.run()
        assert b.fetch()[0].tobytes() == got[i].tobytes(), "row %d" % i
        b.close()
    q.close(); t.close()
    assert len(set(x.tobytes() for x in got)) == 3
    r = subprocess.run(args + ["--numBootstraps", "3"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "--numBootstraps needs --quant" in r.stderr
