"""The variational Bayes method on the device (qm_quant_set_method, qm_quant_exp_digamma, Quant.set_method, EqClasses.quantify,
Bootstrap under VBEM) against the restatement in vb_cases.py.  Tables are filled through add_labels, so most tests need no mapping
at all; the synth_small table is the one the device builds from its own mapping.  The checks are vb_cases.py's, the same the lane
emulation runs (test_vb.py).  Run on the MI355X box: -m gpu."""
import numpy as np
import pytest

import boot_cases as bc
import quant_cases as qc
import vb_cases as vc
from util import pack

pytestmark = pytest.mark.gpu


class ArgError(Exception):
    """QM_E_ARG"""


class StateError(Exception):
    """QM_E_STATE"""


def _call(f, *a, **kw):
    import rapmap_amd as ra
    try:
        return f(*a, **kw)
    except ra.QmError as e:
        if "error -1:" in str(e):
            raise ArgError(str(e))
        if "error -7:" in str(e):
            raise StateError(str(e))
        raise


class DeviceQuant:
    """what vb_cases' env.quant returns: a table (filled through add_labels unless given) and its Quant"""

    def __init__(self, mp, off, tids, cnt, n_txps, eff, table=None):
        import rapmap_amd as ra
        self.own = table is None
        self.t = table if table is not None else ra.EqClasses(mp, expected=64)
        self.q = None
        if self.own and len(off) > 1:
            self.t.add_labels(off, tids, cnt)
        self.q = ra.Quant(self.t, n_txps, eff)
        self.n_txps = self.q.n_txps

    def set_method(self, method="em", prior=None):
        _call(self.q.set_method, method, prior=prior)

    def set_method_code(self, code, prior=None):
        from rapmap_amd.api import _check, lib
        p = None if prior is None else np.ascontiguousarray(prior, dtype=np.float64)
        _call(lambda: _check(lib().qm_quant_set_method(self.q._h, int(code), p.ctypes.data if p is not None and p.size else None)))

    def set_start(self, alpha0=None):
        _call(self.q.set_start, alpha0)

    def run(self, **kw):
        return _call(self.q.run, **kw)

    def fetch(self):
        return self.q.fetch()

    def classes(self):
        return self.q.classes()

    def close(self):
        if self.q is not None:
            self.q.close()
            self.q = None
            if self.own:
                self.t.close()


class DeviceBoot:
    def __init__(self, dq, n_reps):
        import rapmap_amd as ra
        self.b = _call(ra.Bootstrap, dq.q, n_reps)

    def resample(self, seed=0, first_rep=0):
        self.b.resample(seed=seed, first_rep=first_rep)

    def set_counts(self, rep, counts):
        _call(self.b.set_counts, rep, counts)

    def counts(self, rep):
        return _call(self.b.counts, rep)

    def run(self, **kw):
        return _call(self.b.run, **kw)

    def fetch(self):
        return self.b.fetch()

    def close(self):
        self.b.close()


def make_env(mp, table=None):
    import rapmap_amd as ra

    class Env:
        pass
    Env.ArgError, Env.StateError = ArgError, StateError
    Env.quant = staticmethod(lambda off, tids, cnt, n_txps, eff: DeviceQuant(mp, off, tids, cnt, n_txps, eff, table))
    Env.boot = staticmethod(DeviceBoot)
    Env.exp_digamma = staticmethod(lambda x: ra.exp_digamma(x, device=0))
    return Env


@pytest.fixture(scope="module")
def small(synth_small):
    import rapmap_amd as ra
    qi = ra.QuasiIndex(synth_small["idx"])
    mp = ra.QuasiMapper(qi, 0, debug=False)
    q1, o1 = pack(synth_small["reads1"]); q2, o2 = pack(synth_small["reads2"])
    yield {"qi": qi, "mp": mp, "q1": q1, "o1": o1, "q2": q2, "o2": o2}
    mp.close()


@pytest.fixture(scope="module")
def env(small):
    return make_env(small["mp"])


@pytest.fixture(scope="module")
def crafted(env):
    return vc.crafted() + (env,)


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


def test_exp_digamma_bit_for_bit(env):
    vc.check_exp_digamma_bits(env)


def test_against_restatement(table):
    name, (g, eff, env) = table
    vc.check_against_restatement(env, g, eff, name)


def test_single_tid_table(env):
    vc.check_single_tid_table(env)


def test_zero_weight_cases(env):
    vc.check_zero_weight_cases(env)


def test_null_prior_is_zeros(env):
    vc.check_null_prior_is_zeros(env)


def test_invariants(table):
    name, (g, eff, env) = table
    vc.check_invariants(env, g, eff, name)


def test_method_switch(small_table):
    g, eff, env = small_table
    vc.check_method_switch(env, g, eff, "synth_small")


def test_stopping_rule(small_table):
    g, eff, env = small_table
    vc.check_stopping_rule(env, g, eff, "synth_small")


def test_weak_isoform(env):
    vc.check_weak_isoform(env)


def test_boot_slots(env):
    vc.check_boot_slots(env)


def test_boot_against_restatement(table, env):
    name, (g, eff, tenv) = table
    if name == "crafted":
        g, eff = bc.crafted_graph()                                  # (the crafted table's own counts add up to 1.9e14 draws per replicate)
    vc.check_boot_against_restatement(tenv, g, eff, name)


def test_errors_and_lifetime(env):
    vc.check_errors_and_lifetime(env)


def test_python_face(small):
    """Quant.set_method builds the prior from a scalar (per nucleotide: P x the effective lengths Quant was given; per transcript: P);
    EqClasses.quantify takes the same arguments"""
    import rapmap_amd as ra
    L, n, nt = bc.mixed_table()
    off, tids, cnt = qc.table_of(L, n)
    g = qc.Graph(off, tids, cnt, nt)
    eff = qc.random_eff(nt)
    t = ra.EqClasses(small["mp"], expected=64)
    t.add_labels(off, tids, cnt)
    for per in (False, True):
        q = ra.Quant(t, nt, eff)
        q.set_method("vbem", prior=vc.prior_of(2e-2, per, eff, nt))
        q.run(max_iter=12, rel_tol=0.0)
        by_array = q.fetch()
        q.set_start(None)
        q.set_method(method="vbem", prior=2e-2, per_transcript=per)
        q.run(max_iter=12, rel_tol=0.0)
        assert q.fetch().tobytes() == by_array.tobytes()
        q.close()
        assert t.quantify(nt, eff, method="vbem", prior=2e-2, per_transcript=per, max_iter=12, rel_tol=0.0).tobytes() == by_array.tobytes()
        vc.assert_close(by_array, vc.iterate(g, eff, vc.prior_of(2e-2, per, eff, nt), g.uniform_start(), 12), "per_transcript=%s" % per)
    q = ra.Quant(t, nt)                                              # no effective lengths: 1.0 each, the two priors coincide
    q.set_method("vbem")                                             # the default prior
    q.run(max_iter=5, rel_tol=0.0)
    vc.assert_close(q.fetch(), vc.iterate(g, np.ones(nt), np.full(nt, 1e-2), g.uniform_start(), 5), "default prior")
    with pytest.raises(ValueError):
        q.set_method("map")
    with pytest.raises(ValueError):
        q.set_method("vbem", prior=np.ones(nt + 1))
    assert t.quantify(nt, eff, max_iter=12, rel_tol=0.0).tobytes() == t.quantify(nt, eff, method="em", max_iter=12, rel_tol=0.0).tobytes()
    q.close(); t.close()
