"""Inputs and expected answers of the abundance-estimation tests (test_quant.py: lane emulation, test_quant_gpu.py: device).

The model is restated here in numpy float64 over the canonical arrays a table's fetch() returns (label_offsets, tids, counts):
    w_t = alpha_t / e_t      d_c = sum of w_t over t in L_c      r_c = n_c / d_c (0 when d_c < DBL_MIN)
    alpha'_t = w_t * (sum of r_c over the classes that contain t)
np.add.at adds member by member in the order of its index array: ascending as the arrays lie, descending when they are reversed."""
import numpy as np

import eqc_cases as ec

DBL_MIN = float(np.finfo(np.float64).tiny)
DEFAULTS = dict(max_iter=10000, check_every=10, rel_tol=1e-2, min_alpha=1e-8)
ITERS = (1, 2, 25)

# Tolerance of a device (or emulated) alpha against the restatement, relative, for transcripts whose reference alpha is above
# ALPHA_CUT; below the cut the comparison is absolute at ALPHA_CUT * REL_TOL.  It is 64 x the largest relative difference between two
# CPU evaluations of the same input -- the float64 restatement summing members ascending, and the same code summing descending in
# np.longdouble -- at 1, 2 and 25 iterations, with a floor of 1e-13; the factor covers the device's tree-shaped sums against
# numpy's sequential ones.  Measured by measure_tolerance() (profiles/quant/results/tolerance.txt):
#   crafted lists (1 220 classes, 12 768 entries, 4 592 transcripts, longest label 2 500, longest transcript list 266):
#                  1 iteration 9.57e-16, 2 iterations 1.45e-15, 25 iterations 7.79e-15
#   synth_small, default options (the oracle's hits; 1 711 transcripts): 1 iteration 4.24e-16, 2 iterations 4.74e-16, 25 iterations 1.29e-15
#   the largest: 7.79e-15; 64 x that = 4.99e-13, above the floor
ALPHA_CUT = 1e-6
MEASURED_MAX_REL = 7.79e-15
REL_TOL = max(1e-13, 64 * MEASURED_MAX_REL)


class Graph:
    """the canonical arrays of a table as the restatement reads them"""

    def __init__(self, off, tids, cnt, n_txps):
        self.off = np.asarray(off, dtype=np.int64); self.tid = np.asarray(tids, dtype=np.int64); self.cnt = np.asarray(cnt, dtype=np.uint64)
        self.nc = len(self.off) - 1; self.nt = int(n_txps)
        self.cls = np.repeat(np.arange(self.nc, dtype=np.int64), np.diff(self.off))
        self.members = np.bincount(self.tid, minlength=self.nt) if self.tid.size else np.zeros(self.nt, dtype=np.int64)   # classes per transcript
        self.present = self.members > 0
        self.total = int(self.cnt.astype(object).sum()) if self.nc else 0
        self.longest_label = int(np.diff(self.off).max()) if self.nc else 0
        self.longest_list = int(self.members.max()) if self.nt else 0

    def uniform_start(self):
        m = int(self.present.sum())
        return np.where(self.present, float(self.total) / m if m else 0.0, 0.0)


def step(g, eff, alpha, dtype=np.float64, descending=False):
    """one iteration"""
    cls, tid = (g.cls[::-1], g.tid[::-1]) if descending else (g.cls, g.tid)
    w = np.asarray(alpha, dtype=dtype) / np.asarray(eff, dtype=dtype)
    d = np.zeros(g.nc, dtype=dtype)
    np.add.at(d, cls, w[tid])
    skip = d < DBL_MIN
    r = np.where(skip, dtype(0), g.cnt.astype(dtype) / np.where(skip, dtype(1), d))
    s = np.zeros(g.nt, dtype=dtype)
    np.add.at(s, tid, r[cls])
    return w * s


def iterate(g, eff, alpha, n, **kw):
    for _ in range(n):
        alpha = step(g, eff, alpha, **kw)
    return alpha


def rel_change(a0, a1, min_alpha):
    m = a1 > min_alpha
    return float((np.abs(a1[m] - a0[m]) / a1[m]).max()) if m.any() else 0.0


def run(g, eff, alpha, max_iter=DEFAULTS["max_iter"], check_every=DEFAULTS["check_every"], rel_tol=DEFAULTS["rel_tol"], min_alpha=DEFAULTS["min_alpha"]):
    """the stopping rule: the relative change is looked at every check_every-th iteration only -> (alpha, iterations, last relative
    change (-1: never looked at), [(iteration, relative change) of every check])"""
    it, rel, checks = 0, -1.0, []
    if g.nc == 0:
        return alpha, 0, rel, checks
    while it < max_iter:
        a1 = step(g, eff, alpha)
        it += 1
        if rel_tol > 0 and it % check_every == 0:
            rel = rel_change(alpha, a1, min_alpha)
            checks.append((it, rel))
        alpha = a1
        if checks and checks[-1][0] == it and rel < rel_tol:
            break
    return alpha, it, rel, checks


def log_likelihood(g, eff, alpha):
    w = np.asarray(alpha, dtype=np.float64) / eff
    d = np.zeros(g.nc); np.add.at(d, g.cls, w[g.tid])
    return float((g.cnt.astype(np.float64) * np.log(d)).sum())


def roundoff_bound(g):
    """Relative bound on |sum(alpha) - total| / total after an iteration (the device's sums or numpy's, any order): with u = 2^-52,
    d_c is a sum of at most `longest label` terms (relative error <= longest_label * u), r_c adds a division, a transcript's sum
    of r_c has at most `longest list` terms (<= longest_list * u), the product and the next w_t add three roundings, and summing the
    alphas in numpy (pairwise) a few more: every alpha'_t is off by at most (longest_label + longest_list + 8) * u relative, all
    terms are non-negative so the total inherits that relative bound, and 64 - 8 roundings are left for the final sum."""
    return (g.longest_label + g.longest_list + 64) * 2.0 ** -52


def assert_close(got, ref, what=""):
    """every transcript is compared: relatively above the cut, absolutely below it"""
    got = np.asarray(got, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, what
    hi = ref > ALPHA_CUT
    relerr = float((np.abs(got[hi] - ref[hi]) / ref[hi]).max()) if hi.any() else 0.0
    abserr = float(np.abs(got[~hi] - ref[~hi]).max()) if (~hi).any() else 0.0
    print("%s: %d transcripts above the cut, largest relative difference %.3g (tolerance %.3g); %d below, largest absolute difference %.3g" % (
        what, int(hi.sum()), relerr, REL_TOL, int((~hi).sum()), abserr))
    assert relerr <= REL_TOL, "%s: relative difference %.3g > %.3g" % (what, relerr, REL_TOL)
    assert abserr <= ALPHA_CUT * REL_TOL, "%s: absolute difference %.3g below the cut" % (what, abserr)


def measure_tolerance(inputs):
    """{name: {iterations: largest relative difference}} between the float64 ascending and the long-double descending evaluation"""
    out = {}
    for name, (g, eff) in inputs.items():
        a = g.uniform_start(); b = a.astype(np.longdouble)
        res = {}; done = 0
        for n in ITERS:
            a = iterate(g, eff, a, n - done); b = iterate(g, eff, b, n - done, dtype=np.longdouble, descending=True); done = n
            ref = b.astype(np.float64); hi = ref > ALPHA_CUT
            res[n] = float((np.abs(a[hi] - ref[hi]) / ref[hi]).max())
        out[name] = res
    return out


# ---- the crafted inputs
ONE_STEP_SIZES = (1, 2, 4, 8, 16, 64, 128)
ONE_STEP_MEMBERSHIPS = (1, 8, 9, 64, 65, 3000)
ONE_STEP_NTXPS = 5000


def one_step_table(seed=11):
    """(lists, counts, n_txps) of the one-step test.  With eff = 1 and alpha = 1 everywhere, d_c is the label's size, exact in any
    order, and r_c = n_c / size: label sizes are powers of two (r_c a dyadic rational of at most 7 fractional bits), and the one
    label of 9 tids -- the shortest the queue part takes -- has a count that is a multiple of 9 (r_c an integer).  Every alpha'_t
    is then a sum of fewer than 2^12 such numbers below 2^34: exact in float64 whatever the order.
    tid 0 sits in 3 000 classes {0, i}; tids 1 .. 5 in exactly 8, 9, 64, 65 and 1 classes {t, partner}, every partner in that one class
    only; the other labels draw from a pool of their own (tids 4200 .. 4799); n_txps - 1 is a tid; tids 4800 .. 4997 occur nowhere."""
    rng = np.random.default_rng(seed)
    L, n = [], []
    for i in range(1000, 4000):
        L.append([0, i]); n.append(int(rng.integers(1, 1024)))
    nxt = 100
    for t, k in ((1, 8), (2, 9), (3, 64), (4, 65), (5, 1)):
        for _ in range(k):
            L.append([nxt, t]); n.append(int(rng.integers(1, 1024))); nxt += 1          # (given in descending order: the table sorts)
    pool = np.arange(4200, 4800)
    for size in ONE_STEP_SIZES:
        for _ in range(40 if size <= 16 else 6):
            L.append([int(x) for x in rng.choice(pool, size=size, replace=False)]); n.append(int(rng.integers(1, 1024)))
    L.append([int(x) for x in rng.choice(pool, size=9, replace=False)]); n.append(9 * 37)
    L.append([ONE_STEP_NTXPS - 1]); n.append(5)
    L.append([ONE_STEP_NTXPS - 1, 4200]); n.append((1 << 33) + 5)                       # a count beyond 2^32
    order = rng.permutation(len(L))
    return [L[i] for i in order], np.array([n[i] for i in order], dtype=np.uint64), ONE_STEP_NTXPS


def fixed_point_table():
    """two transcripts, classes {A}: 30, {B}: 10, {A, B}: 40; (60, 20) is a fixed point of the iteration"""
    return [[0], [1], [0, 1]], np.array([30, 10, 40], dtype=np.uint64), 2, np.array([60.0, 20.0])


def crafted_table(seed=5):
    """eqc_cases.crafted_lists() without the lists that hold a tid beyond 2^31, tids remapped to their ranks (so they fill
    [0, n_txps) but for five transcripts at the end that occur nowhere), random effective lengths in [50, 5000]
    -> (lists, weights, n_txps, eff)"""
    L, w = ec.crafted_lists()
    keep = [i for i, x in enumerate(L) if ec.BIG not in x]
    L = [L[i] for i in keep]; w = w[keep]
    uniq = np.unique(np.array([t for x in L for t in x], dtype=np.int64))
    L = [[int(r) for r in np.searchsorted(uniq, np.array(x, dtype=np.int64))] if len(x) else [] for x in L]
    n_txps = int(uniq.size) + 5
    eff = np.random.default_rng(seed).uniform(50.0, 5000.0, size=n_txps)
    return L, w, n_txps, eff


def random_eff(n_txps, seed=6):
    return np.random.default_rng(seed).uniform(50.0, 5000.0, size=n_txps)


# ---- the checks both test files run.  solve(off, tids, cnt, n_txps, eff=None, alpha0=None, **run_kw) -> (alpha, iterations,
# last_rel_change, stats): the lane emulation (emu_quant.run) or the device (a table filled through add_labels, then Quant).
def table_of(lists, weights):
    return ec.canonical(ec.expected(lists, weights))


def check_one_step(solve):
    L, n, nt = one_step_table()
    off, tids, cnt = table_of(L, n)
    g = Graph(off, tids, cnt, nt)
    sizes = set(np.diff(off).tolist())
    assert sizes == set(ONE_STEP_SIZES) | {9}                       # group part: 1 .. 8; queue part: 9, 16; more than one stride: 128
    assert int(cnt[np.diff(off) == 9][0]) % 9 == 0
    assert [int(g.members[t]) for t in (5, 1, 2, 3, 4, 0)] == list(ONE_STEP_MEMBERSHIPS)
    assert (g.members == 0).sum() > 0 and g.members[4900] == 0 and g.members[nt - 1] > 0 and int(cnt.max()) > 1 << 32
    ones = np.ones(nt)
    ref = step(g, ones, ones)
    assert np.array_equal(ref, step(g, ones, ones, descending=True)) and np.array_equal(ref, step(g, ones, ones, dtype=np.longdouble).astype(np.float64))   # exact in any order
    got, it, rel, st = solve(off, tids, cnt, nt, None, ones, max_iter=1, rel_tol=0.0)
    assert it == 1 and rel == -1.0
    assert np.array_equal(got, ref), "one step differs in %d transcripts" % int((got != ref).sum())
    assert got[4900] == 0.0 and float(got.sum()) == float(g.total)
    assert (st["classes"], st["entries"], st["present"], st["longest_label"], st["longest_list"]) == (g.nc, tids.size, int(g.present.sum()), 128, 3000)
    assert st["queued_labels"] == int((np.diff(off) > 8).sum()) and st["queued_txps"] == int((g.members > 8).sum())


def check_fixed_point(solve):
    L, n, nt, start = fixed_point_table()
    off, tids, cnt = table_of(L, n)
    for eff in (None, np.array([64.0, 64.0])):
        for iters in (1, 5):
            got, it, _, _ = solve(off, tids, cnt, nt, eff, start, max_iter=iters, rel_tol=0.0)
            assert it == iters and got.tolist() == [60.0, 20.0], (eff, iters, got)


def check_against_restatement(solve, g, eff, what):
    """1, 2 and 25 iterations at rel_tol = 0, from the uniform start"""
    ref = g.uniform_start(); done = 0
    for n in ITERS:
        ref = iterate(g, eff, ref, n - done); done = n
        got, it, rel, _ = solve(g.off, g.tid, g.cnt, g.nt, eff, None, max_iter=n, rel_tol=0.0)
        assert it == n
        assert_close(got, ref, "%s, %d iterations" % (what, n))


def check_invariants(solve, g, eff, what):
    a50, _, _, st = solve(g.off, g.tid, g.cnt, g.nt, eff, None, max_iter=50, rel_tol=0.0)
    bound = roundoff_bound(g)
    assert (st["longest_label"], st["longest_list"]) == (g.longest_label, g.longest_list)
    relsum = abs(float(a50.sum()) - float(g.total)) / float(g.total)
    print("%s: |sum(alpha) - total| / total = %.3g (bound %.3g)" % (what, relsum, bound))
    assert relsum <= bound
    assert not a50[~g.present].any()                                # absent from every label: exactly 0
    a10 = solve(g.off, g.tid, g.cnt, g.nt, eff, None, max_iter=10, rel_tol=0.0)[0]
    a20 = solve(g.off, g.tid, g.cnt, g.nt, eff, None, max_iter=20, rel_tol=0.0)[0]
    l10, l20 = log_likelihood(g, eff, a10), log_likelihood(g, eff, a20)
    print("%s: log-likelihood %.17g at 10 iterations, %.17g at 20" % (what, l10, l20))
    assert l20 >= l10 - bound * abs(l10)


def rel_change_tolerance(rel):
    """what REL_TOL on the alphas means for a relative change |1 - a0 / a1|: a0 and a1 are each within REL_TOL of the restatement's,
    relatively, so their quotient (close to 1) is within 2 * REL_TOL, and so is its distance from 1, absolutely"""
    return 2 * REL_TOL * (1 + rel)


def check_single_tid_classes(solve, g, eff, what):
    """a transcript that occurs only in single-tid classes holds exactly its count after 50 iterations"""
    a50 = solve(g.off, g.tid, g.cnt, g.nt, eff, None, max_iter=50, rel_tol=0.0)[0]
    size = np.diff(g.off)[g.cls]
    multi = np.bincount(g.tid[size > 1], minlength=g.nt) > 0
    alone = g.present & ~multi
    own = np.zeros(g.nt, dtype=np.float64); m1 = size == 1
    np.add.at(own, g.tid[m1], g.cnt.astype(np.float64)[g.cls[m1]])
    ref = iterate(g, eff, g.uniform_start(), 50)
    off_by = np.abs(a50[alone] - own[alone]) / np.where(own[alone] > 0, own[alone], 1.0)
    ref_by = np.abs(ref[alone] - own[alone]) / np.where(own[alone] > 0, own[alone], 1.0)
    print("%s: %d transcripts occur in single-tid classes only; %d of them do not hold exactly their count (largest relative miss %.3g); "
          "the restatement: %d (%.3g)" % (what, int(alone.sum()), int((off_by > 0).sum()), float(off_by.max()) if alone.any() else 0.0,
                                          int((ref_by > 0).sum()), float(ref_by.max()) if alone.any() else 0.0))
    assert np.array_equal(a50[alone], own[alone])
    return int(alone.sum())


def check_stopping_rule(solve, g, eff, what):
    got, it, rel, _ = solve(g.off, g.tid, g.cnt, g.nt, eff, None, **DEFAULTS)
    ref, rit, rrel, checks = run(g, eff, g.uniform_start(), **DEFAULTS)
    print("%s: stopped after %d iterations at %.17g (restatement: %d at %.17g)" % (what, it, rel, rit, rrel))
    ce, tol = DEFAULTS["check_every"], DEFAULTS["rel_tol"]
    assert it > 0 and it % ce == 0 and 0 <= rel < tol
    assert abs(it - rit) <= ce
    if it != rit:                                                   # a check that fell within roundoff of the threshold went the other way
        early = dict(checks)[min(it, rit)]
        assert abs(early - tol) <= rel_change_tolerance(tol), (it, rit, early)
    else:
        assert abs(rel - rrel) <= rel_change_tolerance(rrel), (rel, rrel)
        assert_close(got, ref, what + ", converged")


def check_errors_and_edges(solve, arg_error):
    import pytest
    off, tids, cnt = table_of([[0, 3], [7]], None)
    with pytest.raises(arg_error):
        solve(off, tids, cnt, 7, None, None, max_iter=1)             # tid 7 with seven transcripts
    solve(off, tids, cnt, 8, None, None, max_iter=1)
    for bad in (0.0, -1.0, np.inf, np.nan):
        e = np.ones(8); e[5] = bad
        with pytest.raises(arg_error):
            solve(off, tids, cnt, 8, e, None, max_iter=1)
    for bad in (-1e-300, np.inf, np.nan):
        a = np.ones(8); a[2] = bad
        with pytest.raises(arg_error):
            solve(off, tids, cnt, 8, None, a, max_iter=1)
    got, it, rel, st = solve(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint64), 6, None, None, **DEFAULTS)
    assert it == 0 and got.tolist() == [0.0] * 6 and st["classes"] == 0
    got, it, rel, st = solve(off, tids, cnt, 8, None, None, max_iter=0)
    assert it == 0 and got.tolist() == [2.0 / 3, 0, 0, 2.0 / 3, 0, 0, 0, 2.0 / 3]   # the uniform start: total 2 over M = 3
