"""Inputs, the numpy restatement and the checks of the bootstrap tests (test_boot.py: lane emulation, test_boot_gpu.py: device).

The draw is restated here word for word (Philox4x32-10, two draws per call, the high half of u * N, the class by the prefix sums), so
the counts of a replicate can be demanded EQUAL; the per-replicate EM is quant_cases' (step / iterate / run) over that replicate's counts.

Both test files hand the checks an `env`:
    env.make(off, tids, cnt, n_txps, eff, n_reps) -> an object with the methods of rapmap_amd.Bootstrap plus classes() (the snapshot's
        class side in snapshot order: Quant.classes() on the device) and close()
    env.solve(off, tids, cnt, n_txps, eff, alpha0, **run_kw) -> quant_cases' solve(): Quant itself
    env.ArgError, env.StateError: what QM_E_ARG and QM_E_STATE come out as."""
import numpy as np
import pytest

import quant_cases as qc

M32 = np.uint64(0xffffffff)
S32 = np.uint64(32)
TILE = 16                   # BOOT_TILE: replicates per wavefront
LONG = 32                   # BOOT_LONG: a longer row is walked by a wavefront of its own

# Tolerance of a replicate's alpha against the restatement: quant_cases.assert_close's, i.e. 64 x the largest relative difference between
# two CPU evaluations (float64 ascending / long double descending).  measure_tolerance taken again on REPLICATE tables (17 replicates of
# the crafted table and of synth_small, seed 7; profiles/boot/measure_tolerance.py, profiles/boot/results/tolerance.txt) gives the figure
# below; the bound used is the larger of the two, defined the same way.
MEASURED_MAX_REL_REPLICATES = 4.78e-15
REL_TOL = max(qc.REL_TOL, 64 * MEASURED_MAX_REL_REPLICATES)


# ---- the restatement
def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over arrays (or scalars) of 32-bit values held in uint64 -> (x0, x1, x2, x3)"""
    c0, c1, c2, c3, k0, k1 = (np.atleast_1d(np.asarray(v, dtype=np.uint64)) & M32 for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0; p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & M32, (p0 >> S32) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32; k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def mulhi64(a, b):
    """the high 64 bits of a * b, a an array of uint64, b an integer below 2^64"""
    a = np.asarray(a, dtype=np.uint64); b = np.uint64(int(b))
    al, ah, bl, bh = a & M32, a >> S32, b & M32, b >> S32
    t = ah * bl + ((al * bl) >> S32)
    return ah * bh + (t >> S32) + ((al * bh + (t & M32)) >> S32)


def draw_classes(cnt, seed, rep):
    """the class of every draw j = 0 .. N - 1 of replicate number `rep`"""
    cnt = np.asarray(cnt, dtype=np.uint64)
    n = int(cnt.astype(object).sum()) if cnt.size else 0
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    seed, rep = int(seed) & (2 ** 64 - 1), int(rep) & (2 ** 64 - 1)
    k = np.arange((n + 1) // 2, dtype=np.uint64)
    x0, x1, x2, x3 = philox(k & M32, k >> S32, rep & 0xffffffff, rep >> 32, seed & 0xffffffff, seed >> 32)
    u = np.empty(2 * k.size, dtype=np.uint64)
    u[0::2] = x0 | (x1 << S32); u[1::2] = x2 | (x3 << S32)
    p = mulhi64(u[:n], n)
    return np.searchsorted(np.cumsum(cnt), p, side="right").astype(np.int64)       # cum[c] <= p < cum[c + 1]


def draw_counts(cnt, seed, rep):
    return np.bincount(draw_classes(cnt, seed, rep), minlength=len(cnt)).astype(np.uint64)


PHILOX_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def assert_close(got, ref, what=""):
    """quant_cases.assert_close with this file's REL_TOL"""
    got = np.asarray(got, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, what
    hi = ref > qc.ALPHA_CUT
    relerr = float((np.abs(got[hi] - ref[hi]) / ref[hi]).max()) if hi.any() else 0.0
    abserr = float(np.abs(got[~hi] - ref[~hi]).max()) if (~hi).any() else 0.0
    print("%s: %d above the cut, largest relative difference %.3g (tolerance %.3g); %d below, largest absolute difference %.3g" % (
        what, int(hi.sum()), relerr, REL_TOL, int((~hi).sum()), abserr))
    assert relerr <= REL_TOL, "%s: relative difference %.3g > %.3g" % (what, relerr, REL_TOL)
    assert abserr <= qc.ALPHA_CUT * REL_TOL, "%s: absolute difference %.3g below the cut" % (what, abserr)


# ---- the tables
def seven_class_table():
    """eight classes with counts [1, 0, 7000, 12, 300, 5000, 2, 7686]; the one of count 0 cannot be in a table, so seven: N = 20 001, odd"""
    lists = [[0], [1, 2], [2], [0, 3], [4, 5, 6], [1], [3, 4, 7]]
    return lists, np.array([1, 7000, 12, 300, 5000, 2, 7686], dtype=np.uint64), 9


def mixed_table(seed=3):
    """300 classes with counts 1 .. 300 (N = 45 150) over 140 transcripts: labels of 1 .. 6 tids, one label of 40 (more than BOOT_LONG) and
    one of 33, tid 0 in 60 classes {0, t} (a transcript list of more than BOOT_LONG), tids 120 .. 129 in single-tid classes only, tids
    130 .. 139 nowhere"""
    rng = np.random.default_rng(seed)
    seen, L = set(), []

    def put(x):
        x = tuple(sorted(set(int(v) for v in x)))
        if x in seen or not x:
            return False
        seen.add(x); L.append(list(x))
        return True
    put(range(60, 100)); put(range(80, 113))
    for t in range(120, 130):
        put([t])
    for t in range(1, 61):
        put([0, t])
    while len(L) < 300:
        put(rng.choice(np.arange(1, 120), size=int(rng.integers(1, 7)), replace=False))
    order = rng.permutation(300)
    return [L[i] for i in order], np.arange(1, 301, dtype=np.uint64), 140


def crafted_graph():
    """quant_cases.crafted_table() with its labels, transcripts and effective lengths as they are and every count n replaced by
    1 + n % 7: the table's own counts add up to 1.9e14 (one of them is beyond 2^40), and a resample is N draws per replicate.
    N is then about 12 000 -> (graph over the canonical arrays, eff)"""
    L, w, nt, eff = qc.crafted_table()
    off, tids, cnt = qc.table_of(L, w)
    return qc.Graph(off, tids, np.uint64(1) + cnt % np.uint64(7), nt), eff


def graph_of(b, counts=None):
    """quant_cases.Graph over the snapshot order of b, with `counts` in place of the snapshot's"""
    off, tids, cnt = b.classes()
    return qc.Graph(off, tids, cnt if counts is None else counts, b.n_txps)


# ---- the checks both test files run
def check_philox_restatement():
    for ctr, key, out in PHILOX_ANSWERS:
        got = philox(*ctr, *key)
        assert tuple(int(x[0]) for x in got) == out, (ctr, key, [hex(int(x[0])) for x in got])


def check_draws_exact(env):
    tables = {"seven": seven_class_table(), "one": ([[2]], np.array([1], dtype=np.uint64), 4), "empty": ([], np.zeros(0, dtype=np.uint64), 5),
              "mixed": mixed_table()}
    for name, (L, n, nt) in tables.items():
        off, tids, cnt = qc.table_of(L, n) if L else (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint64))
        total = int(cnt.sum())
        pair, lone = env.make(off, tids, cnt, nt, None, 2), env.make(off, tids, cnt, nt, None, 1)
        soff, stids, scnt = pair.classes()
        assert len(soff) == len(off) and sorted(scnt.tolist()) == sorted(cnt.tolist())
        assert sorted(tuple(stids[soff[i]:soff[i + 1]].tolist()) + (int(scnt[i]),) for i in range(len(scnt))) == \
            sorted(tuple(tids[off[i]:off[i + 1]].tolist()) + (int(cnt[i]),) for i in range(len(cnt))), "classes() is not the table"
        for seed in (0, 12345, 2 ** 64 - 1):
            pair.resample(seed=seed, first_rep=0); lone.resample(seed=seed, first_rep=2 ** 32 + 3)
            for b, slot, rep in ((pair, 0, 0), (pair, 1, 1), (lone, 0, 2 ** 32 + 3)):
                got = b.counts(slot)
                assert got.dtype == np.uint64 and int(got.sum()) == total, (name, seed, rep)
                assert np.array_equal(got, draw_counts(scnt, seed, rep)), "%s, seed %d, replicate %d: counts differ from the restatement" % (name, seed, rep)
        if name == "empty":
            it, rel = lone.run(max_iter=3, rel_tol=0.0)
            assert it.tolist() == [0] and lone.fetch().tolist() == [[0.0] * nt]
        if name == "one":
            it, rel = lone.run(max_iter=3, rel_tol=0.0)
            assert it.tolist() == [3] and lone.fetch().tolist() == [[0.0, 0.0, 1.0, 0.0]]
        pair.close(); lone.close()


def check_slots_do_not_matter(env):
    """replicate number 37 alone and in slot 7 of 15, 16, 17 and 33 replicates that begin at number 30"""
    L, n, nt = mixed_table()
    off, tids, cnt = qc.table_of(L, n)
    eff = qc.random_eff(nt)
    tol_kw = dict(max_iter=5000, rel_tol=1e-2, check_every=3)          # (replicates of this table stop after 400 .. 1 800 iterations)
    alone = env.make(off, tids, cnt, nt, eff, 1)
    alone.resample(seed=99, first_rep=37)
    c0 = alone.counts(0)
    it, rel = alone.run(max_iter=25, rel_tol=0.0)
    assert it.tolist() == [25] and rel.tolist() == [-1.0]
    a0 = alone.fetch()[0]
    alone.resample(seed=99, first_rep=37)
    it0, rel0 = alone.run(**tol_kw)
    b0 = alone.fetch()[0]
    assert 0 < it0[0] < 5000 and it0[0] % 3 == 0 and 0 <= rel0[0] < 1e-2
    alone.close()
    for n_reps in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        b = env.make(off, tids, cnt, nt, eff, n_reps)
        b.resample(seed=99, first_rep=30)
        assert np.array_equal(b.counts(7), c0)
        it, rel = b.run(max_iter=25, rel_tol=0.0)
        assert it.tolist() == [25] * n_reps
        assert b.fetch()[7].tobytes() == a0.tobytes(), "%d replicates: alpha of replicate 37 differs after 25 iterations" % n_reps
        b.resample(seed=99, first_rep=30)
        it, rel = b.run(**tol_kw)
        a = b.fetch()
        print("%d replicates: iterations %s" % (n_reps, it.tolist()))
        assert it[7] == it0[0] and rel[7] == rel0[0] and a[7].tobytes() == b0.tobytes(), "%d replicates: the stop of replicate 37 differs" % n_reps
        assert ((it > 0) & (it % 3 == 0) & (rel >= 0) & (rel < 1e-2)).all()
        if n_reps == 2 * TILE + 1:
            assert len(set(it.tolist())) > 1, "every replicate stopped at the same check: the freeze is not exercised"
            it2, rel2 = b.run(**tol_kw)                              # everything is done: a later run does nothing
            assert it2.tolist() == [0] * n_reps and np.array_equal(rel2, rel) and b.fetch().tobytes() == a.tobytes()
        b.close()


def check_one_step(env):
    """quant_cases.one_step_table() in all of 17 replicates, replicate 5 with doubled counts.  There is no start to set here: a replicate
    starts from v = total / M, so the effective lengths are v everywhere and the weights 1.0 (2.0 in replicate 5) exactly -- the sums are
    then exact in any order, as in quant_cases.check_one_step."""
    L, n, nt = qc.one_step_table()
    off, tids, cnt = qc.table_of(L, n)
    g0 = qc.Graph(off, tids, cnt, nt)
    v = float(g0.total) / int(g0.present.sum())
    eff = np.full(nt, v)
    b = env.make(off, tids, cnt, nt, eff, 17)
    scnt = b.classes()[2]
    for rep in range(17):
        b.set_counts(rep, scnt * np.uint64(2) if rep == 5 else scnt)
    assert np.array_equal(b.counts(5), scnt * np.uint64(2)) and np.array_equal(b.counts(16), scnt)
    it, rel = b.run(max_iter=1, rel_tol=0.0)
    assert it.tolist() == [1] * 17 and rel.tolist() == [-1.0] * 17
    got = b.fetch()
    for rep in range(17):
        g = graph_of(b, scnt * np.uint64(2) if rep == 5 else scnt)
        start = g.uniform_start()
        assert set(np.unique(start / eff).tolist()) == {0.0, 2.0 if rep == 5 else 1.0}
        ref = qc.step(g, eff, start)
        assert np.array_equal(ref, qc.step(g, eff, start, descending=True))       # exact in any order
        assert np.array_equal(got[rep], ref), "replicate %d: one step differs in %d transcripts" % (rep, int((got[rep] != ref).sum()))
        assert float(got[rep].sum()) == float(g.total) and got[rep][4900] == 0.0
    b.close()


def check_fixed_point(env):
    """quant_cases.fixed_point_table(): (60, 20) is a fixed point.  A replicate cannot be started there (the start is uniform: (40, 40)),
    but on this table the iteration is alpha_A' = 30 + alpha_A / 2, every step exact in float64 while 60 - 20 * 2^-k has the bits for it:
    it arrives at (60, 20) exactly and then stays -- in every replicate that holds the table's counts, whatever its neighbours hold."""
    L, n, nt, fixed = qc.fixed_point_table()
    off, tids, cnt = qc.table_of(L, n)
    b = env.make(off, tids, cnt, nt, None, 3)
    scnt = b.classes()[2]
    b.set_counts(0, scnt); b.set_counts(1, scnt * np.uint64(3)); b.set_counts(2, scnt)
    b.run(max_iter=80, rel_tol=0.0)
    a = b.fetch()
    assert a[0].tolist() == fixed.tolist() and a[2].tolist() == fixed.tolist() and a[1].tolist() == (3 * fixed).tolist(), a
    for iters in (1, 5):
        b.run(max_iter=iters, rel_tol=0.0)
        assert b.fetch().tobytes() == a.tobytes()
    b.close()


def check_against_restatement(env, g, eff, what, seed=7, n_reps=17):
    """17 resampled replicates after 1, 2 and 25 iterations against quant_cases.iterate on each replicate's counts; then the single-tid
    rule; then a replicate given the ORIGINAL counts against Quant itself"""
    b = env.make(g.off, g.tid, g.cnt, g.nt, eff, n_reps)
    b.resample(seed=seed)
    gs = [graph_of(b, b.counts(rep)) for rep in range(n_reps)]
    assert all(x.total == g.total for x in gs) and len(set(x.cnt.tobytes() for x in gs)) == n_reps
    refs = [x.uniform_start() for x in gs]; done = 0
    for n in qc.ITERS:
        it, _ = b.run(max_iter=n - done, rel_tol=0.0)
        assert it.tolist() == [n - done] * n_reps
        got = b.fetch()
        for rep in range(n_reps):
            refs[rep] = qc.iterate(gs[rep], eff, refs[rep], n - done)
            assert_close(got[rep], refs[rep], "%s, replicate %d, %d iterations" % (what, rep, n))
        done = n
    # single-tid rule: a transcript that occurs in one-tid classes only holds exactly its replicate count
    g0 = gs[0]
    size = np.diff(g0.off)[g0.cls]
    alone = g0.present & ~(np.bincount(g0.tid[size > 1], minlength=g0.nt) > 0)
    for rep in range(n_reps):
        own = np.zeros(g0.nt); m1 = size == 1
        np.add.at(own, g0.tid[m1], gs[rep].cnt.astype(np.float64)[g0.cls[m1]])
        assert np.array_equal(got[rep][alone], own[alone]), "%s, replicate %d: a transcript of single-tid classes does not hold its count" % (what, rep)
    print("%s: %d transcripts occur in single-tid classes only" % (what, int(alone.sum())))
    # the original counts in slot 3: Quant's own answer (slot 2 keeps its resampled ones and goes on beside it)
    b.set_counts(3, b.classes()[2])
    for n in (25,):
        b.run(max_iter=n, rel_tol=0.0)
        ref, it, _, _ = env.solve(g.off, g.tid, g.cnt, g.nt, eff, None, max_iter=n, rel_tol=0.0)
        assert it == n
        assert_close(b.fetch()[3], ref, "%s, the original counts against Quant, %d iterations" % (what, n))
    b.close()
    return int(alone.sum())


def check_invariants(env, g, eff, what, seed=8, n_reps=5):
    b = env.make(g.off, g.tid, g.cnt, g.nt, eff, n_reps)
    b.resample(seed=seed)
    b.run(max_iter=50, rel_tol=0.0)
    a = b.fetch()
    bound = qc.roundoff_bound(g)
    for rep in range(n_reps):
        relsum = abs(float(a[rep].sum()) - float(g.total)) / float(g.total)
        print("%s, replicate %d: |sum(alpha) - N| / N = %.3g (bound %.3g)" % (what, rep, relsum, bound))
        assert relsum <= bound
        assert not a[rep][~g.present].any()                          # absent from every label: exactly 0
    b.close()


def check_zero_count_class(env):
    """a class whose replicate count is 0 changes nothing else: the replicate agrees with the restatement on the table WITHOUT that class"""
    L, n, nt = mixed_table()
    off, tids, cnt = qc.table_of(L, n)
    eff = qc.random_eff(nt, seed=9)
    b = env.make(off, tids, cnt, nt, eff, 2)
    soff, stids, scnt = b.classes()
    g = graph_of(b)
    size = np.diff(soff)
    victim = next(c for c in range(g.nc) if size[c] > 1 and (g.members[stids[soff[c]:soff[c + 1]]] > 1).all())     # (M stays what it was)
    zeroed = scnt.copy(); zeroed[victim] = 0
    b.set_counts(0, scnt); b.set_counts(1, zeroed)
    assert b.counts(1)[victim] == 0
    b.run(max_iter=25, rel_tol=0.0)
    a = b.fetch()
    keep = np.arange(g.nc) != victim
    lists = [stids[soff[c]:soff[c + 1]] for c in range(g.nc) if keep[c]]
    g1 = qc.Graph(np.concatenate([[0], np.cumsum([len(x) for x in lists])]), np.concatenate(lists), scnt[keep], nt)
    assert np.array_equal(g1.present, g.present)
    assert_close(a[1], qc.iterate(g1, eff, g1.uniform_start(), 25), "without class %d" % victim)
    assert_close(a[0], qc.iterate(g, eff, g.uniform_start(), 25), "with it")
    b.close()


def scheme_statistics(counts_of, cnt, n_reps=64):
    """the seven-class table (cnt: its counts in the order counts_of gives them), 64 replicates: the mean count of every class against
    n_c, in standard errors sqrt(N p (1 - p) / 64)"""
    cnt = np.asarray(cnt).astype(np.float64)
    n = cnt.sum(); p = cnt / n
    reps = np.stack([counts_of(r) for r in range(n_reps)]).astype(np.float64)
    assert (reps.sum(axis=1) == n).all()
    z = np.abs(reps.mean(axis=0) - cnt) / np.sqrt(n * p * (1 - p) / n_reps)
    distinct = len(set(r.tobytes() for r in reps))
    print("largest deviation of a class mean: %.3g standard errors; %d distinct replicates of %d" % (float(z.max()), distinct, n_reps))
    assert z.max() <= 5.0 and distinct == n_reps
    return float(z.max())


def check_errors(env):
    L, n, nt = seven_class_table()
    off, tids, cnt = qc.table_of(L, n)
    with pytest.raises(env.ArgError):
        env.make(off, tids, cnt, nt, None, 0)
    b = env.make(off, tids, cnt, nt, None, 3)
    with pytest.raises(env.StateError):
        b.run(max_iter=1)
    for rep in (-1, 3):
        with pytest.raises(env.ArgError):
            b.set_counts(rep, cnt)
        with pytest.raises(env.ArgError):
            b.counts(rep)
    b.set_counts(1, b.classes()[2])                                  # one slot with counts is enough to run; the others hold none and stay 0
    it, rel = b.run(max_iter=2, rel_tol=0.0)
    assert it.tolist() == [2, 2, 2]
    a = b.fetch()
    assert not a[0].any() and not a[2].any() and abs(a[1].sum() - float(cnt.sum())) < 1e-6
    b.close()


def check_determinism(env):
    L, n, nt = mixed_table()
    off, tids, cnt = qc.table_of(L, n)
    eff = qc.random_eff(nt)
    out = []
    for _ in range(2):
        b = env.make(off, tids, cnt, nt, eff, 5)
        b.resample(seed=4, first_rep=11)
        it, rel = b.run(max_iter=200, rel_tol=1e-2, check_every=4)
        out.append((np.stack([b.counts(r) for r in range(5)]).tobytes(), it.tobytes(), rel.tobytes(), b.fetch().tobytes()))
        b.close()
    assert out[0] == out[1]
