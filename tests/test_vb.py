"""The variational Bayes method without a GPU: the device code (rapmap_amd/csrc/qm_quant.inl, qm_boot.inl) and both drivers under
the lane emulation (tests/emu/qm_emu_vb.cpp), the restatement of E against mpmath, the records behind the two tolerances, the CLI's
argument check.  The checks are vb_cases.py's, the same the device runs (test_vb_gpu.py); here the synth_small table comes from the
oracle's hits instead of the device's."""
import subprocess
import sys

import numpy as np
import pytest

import eqc_cases as ec
import quant_cases as qc
import vb_cases as vc
from conftest import ROOT, load_oracle
from util import pack


@pytest.fixture(scope="module")
def env():
    import emu_vb
    emu_vb._lib()

    class Env:
        ArgError, StateError = emu_vb.ArgError, emu_vb.StateError
        quant = staticmethod(emu_vb.Quant)
        boot = staticmethod(emu_vb.Boot)
        exp_digamma = staticmethod(emu_vb.exp_digamma)
    return Env


@pytest.fixture(scope="module")
def crafted():
    return vc.crafted()


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


def test_emulated_exp_digamma_bit_for_bit(env):
    vc.check_exp_digamma_bits(env)


def test_exp_digamma_is_digamma():
    """the restatement (hence, by the test above, the device function) against mpmath at 50 digits"""
    pytest.importorskip("mpmath")
    (ge1, at1), (lt1, at0) = vc.measure_accuracy()
    print("largest relative error of E: %.3g at x = %.17g (x >= 1), %.3g at x = %.17g (x < 1, E > 1e-300)" % (ge1, at1, lt1, at0))
    assert ge1 <= vc.ACC_BOUND_GE1 and lt1 <= vc.ACC_BOUND_LT1
    assert vc.ACC_MEASURED_GE1 * 0.9 <= ge1 <= vc.ACC_MEASURED_GE1 * 1.1 and vc.ACC_MEASURED_LT1 * 0.9 <= lt1 <= vc.ACC_MEASURED_LT1 * 1.1   # the record is this measurement


def test_crafted_lists_cover_both_paths(crafted):
    vc.check_crafted_covers(crafted[0])


def test_tolerance_record_matches_the_constant(crafted, small):
    """the measurement behind vb_cases.REL_TOL, taken again"""
    m = vc.measure_tolerance({"crafted": crafted, "synth_small": small})
    for name, by_prior in m.items():
        for pname, res in by_prior.items():
            print("%s, prior %s: %s" % (name, pname, ", ".join("%d iterations %.3g" % kv for kv in res.items())))
    worst = max(v for by_prior in m.values() for res in by_prior.values() for v in res.values())
    print("largest CPU-to-CPU difference of the variational step: %.3g" % worst)
    assert vc.MEASURED_MAX_REL_VB * 0.9 <= worst <= vc.MEASURED_MAX_REL_VB * 1.1
    assert vc.REL_TOL == (qc.REL_TOL if vc.MEASURED_MAX_REL_VB <= qc.MEASURED_MAX_REL else 64 * vc.MEASURED_MAX_REL_VB)


def test_emulated_against_restatement(env, table):
    name, (g, eff) = table
    vc.check_against_restatement(env, g, eff, name)


def test_emulated_single_tid_table(env):
    vc.check_single_tid_table(env)


def test_emulated_zero_weight_cases(env):
    vc.check_zero_weight_cases(env)


def test_emulated_null_prior_is_zeros(env):
    vc.check_null_prior_is_zeros(env)


def test_emulated_invariants(env, table):
    name, (g, eff) = table
    vc.check_invariants(env, g, eff, name)


def test_emulated_method_switch(env, small):
    vc.check_method_switch(env, small[0], small[1], "synth_small")


def test_emulated_stopping_rule(env, small):
    vc.check_stopping_rule(env, small[0], small[1], "synth_small")


def test_emulated_weak_isoform(env):
    vc.check_weak_isoform(env)


def test_emulated_boot_slots(env):
    vc.check_boot_slots(env)


def test_emulated_boot_against_restatement(env, table):
    name, (g, eff) = table
    if name == "crafted":
        import boot_cases as bc
        g, eff = bc.crafted_graph()                                  # (the crafted table's own counts add up to 1.9e14 draws per replicate)
    vc.check_boot_against_restatement(env, g, eff, name)


def test_emulated_errors_and_lifetime(env):
    vc.check_errors_and_lifetime(env)


def test_cli_rejects_vb_without_quant():
    for extra, msg in ((["--quantVB"], "--quantVB needs --quant"), (["--quant", "q.sf", "--quantVB", "--quantVBPrior", "-1"], "--quantVBPrior")):
        r = subprocess.run([sys.executable, "-m", "rapmap_amd", "quasimap", "-i", "nowhere", "-r", "reads.fq"] + extra,
                           cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 2 and msg in r.stderr, r.stderr
