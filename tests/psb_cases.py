"""Inputs, the restatements and the checks of the positional bias tests (test_pos_bias.py: lane emulation and the host function,
test_pos_bias_gpu.py: device).  Everything here is exact: integer counts, and floats compared bit for bit.

A WORLD is gcb_cases' ({"text", "off", "lens"}); the model looks at the lengths only.  cls / bin_of / classify / expect / ratios /
eff_lens restate the model of include/qmap_mi355.h in Python integers and numpy; expect goes over every position of every
transcript (no closed form), eff_lens spells out the order of every float sum.  A check takes the world and `new(max_len,
max_blocks)`, which makes an object over that world with add_hits / add_counts / counts / stat / expect / eff_lens / position /
clear / close -- rapmap_amd.PosBias on the device, emu_psb.EmuPsb under the lane emulation."""
import numpy as np

import gcb_cases as gc
import sqb_cases as sq
from rapmap_amd.api import HIT_DTYPE

CLASSES, POS, BINS, SHAPE = 5, 20, 200, (2, 5, 20)
BOUNDS = (791, 1265, 1707, 2433)
CATS = gc.CATS                                                       # the GC sweep's seven categories: the gate is the same
STATS = gc.STATS
# each class bound and its neighbour, each tile edge, fewer than 20 positions
LENS = (1, 2, 19, 20, 21, 39, 40, 41, 63, 64, 65, 127, 128, 129, 791, 792, 1265, 1266, 1707, 1708, 2433, 2434, 5000)


def crafted_seqs():
    rng = np.random.default_rng(2026)
    return [gc._rand_seq(rng, n) for n in LENS]


# ---- restatements

def cls(L):
    for c, b in enumerate(BOUNDS):
        if L <= b:
            return c
    return 4


def bin_of(x, L):
    assert 0 <= x < L
    return (20 * int(x)) // int(L)


def edge(b, L):
    """B_b = ceil(b L / 20)"""
    return -((-b * int(L)) // 20)


def bins_of(L):
    """the bin of every position of a transcript of L characters, int64[L] (Python integers underneath: 20 x stays exact)"""
    return (20 * np.arange(L, dtype=np.int64)) // L


def probe(world, tids, positions):
    """int32[n][2]: what qm_psb_position answers"""
    T = world["lens"].size
    out = np.full((len(tids), 2), -1, dtype=np.int32)
    for i, (t, p) in enumerate(zip(tids, positions)):
        t, p = int(t), int(p)
        if t < T and 0 <= p < int(world["lens"][t]):
            L = int(world["lens"][t])
            out[i] = (cls(L), bin_of(p, L))
    return out


def classify(world, hit_offsets, hits, max_len):
    """-> (obs uint64[2][5][20], stats): every unit in the first category whose condition holds"""
    off = np.asarray(hit_offsets, dtype=np.int64)
    n = len(off) - 1
    cnt = np.diff(off)
    st = dict.fromkeys(STATS, 0)
    st["units"] = n
    st["unmapped"] = int(np.count_nonzero(cnt == 0)); st["multi"] = int(np.count_nonzero(cnt >= 2))
    obs = np.zeros(SHAPE, dtype=np.uint64)
    one = off[:-1][cnt == 1]
    if one.size:
        h = np.asarray(hits)[one]
        fl = h["frag_len"].astype(np.int64)
        not_paired = h["mate_status"] != 3
        same = ~not_paired & (h["fwd"] == h["mate_is_fwd"])
        oor = ~not_paired & ~same & ((fl == 0) | (fl > max_len))
        rest = ~not_paired & ~same & ~oor
        st["not_paired"] = int(not_paired.sum()); st["same_strand"] = int(same.sum()); st["out_of_range"] = int(oor.sum())
        T = world["lens"].size
        for r, f in zip(h[rest], fl[rest]):
            t = int(r["tid"]); s = min(max(int(r["pos"]), 0), max(int(r["mate_pos"]), 0)); e = s + int(f)
            if t >= T or e > int(world["lens"][t]):
                st["overhang"] += 1; continue
            L = int(world["lens"][t]); c = cls(L)
            st["used"] += 1
            obs[0, c, bin_of(s, L)] += np.uint64(1); obs[1, c, bin_of(e - 1, L)] += np.uint64(1)
    assert sum(st[k] for k in CATS) == n and int(obs[0].sum()) == st["used"] == int(obs[1].sum())
    return obs, st


def placements(lens, counts):
    """S_t = (L_t + 1) P[m'] - Q[m'], m' = min(L_t, m), in Python integers"""
    c = [int(x) for x in counts]; m = len(c) - 1
    P = sq.prefix(c); Q = [0] * len(c)
    for l in range(1, len(c)):
        Q[l] = Q[l - 1] + l * c[l]
    return [(int(L) + 1) * P[min(int(L), m)] - Q[min(int(L), m)] for L in lens]


def expect(world, counts, q):
    """(exp uint64[2][5][20] in Python integers' arithmetic, the total sum_t q_t S_t both ends must reach): BY BRUTE FORCE, a term per
    position -- a start s carries P[min(m, L - s)], a last position i carries P[min(m, i + 1)]"""
    P = sq.prefix(counts); m = len(P) - 1
    Pa = np.array(P, dtype=object)
    ex = np.zeros(SHAPE, dtype=object)
    for t, L in enumerate(int(x) for x in world["lens"]):
        qt = int(q[t])
        if not qt:
            continue
        x = np.arange(L, dtype=np.int64); b = bins_of(L); c = cls(L)
        np.add.at(ex[0, c], b, Pa[np.minimum(m, L - x)] * qt)
        np.add.at(ex[1, c], b, Pa[np.minimum(m, x + 1)] * qt)
    total = sum(int(a) * s for a, s in zip(q, placements(world["lens"], counts)))
    assert total < 2 ** 64
    return ex.astype(np.uint64), total


def assert_two_ends(ex, total, what=""):
    """both ends sum to sum_t q_t S_t"""
    for e in (0, 1):
        assert sum(int(v) for v in np.asarray(ex)[e].ravel()) == total, (what, e)


def ratios(obs, ex):
    obs = np.asarray(obs, dtype=np.uint64).reshape(SHAPE); ex = np.asarray(ex, dtype=np.uint64).reshape(SHAPE)
    R = np.ones(SHAPE, dtype=np.float64)
    for e in (0, 1):
        for c in range(CLASSES):
            so = sum(int(v) for v in obs[e, c]); se = sum(int(v) for v in ex[e, c])
            if not so or not se:
                continue
            for b in range(POS):
                po = np.float64(int(obs[e, c, b]) + 1) / np.float64(so + 20)
                pe = np.float64(int(ex[e, c, b]) + 1) / np.float64(se + 20)
                R[e, c, b] = min(max(po / pe, np.float64(0.25)), np.float64(4.0))
    return R


def eff_lens(lens, counts, R):
    """e' float64[T] in the header's order: per start ascending l, a product and an addition each; 64 starts by the tree
    (sqb_cases.tile_sums); a transcript's tiles ascending"""
    R = np.asarray(R, dtype=np.float64).reshape(SHAPE)
    c = [int(x) for x in counts]; m = len(c) - 1; P = sq.prefix(c)
    out = np.zeros(len(lens), dtype=np.float64)
    for t, L in enumerate(int(x) for x in lens):
        M = P[min(L, m)]
        if not M:
            out[t] = float(L); continue
        b = bins_of(L); k = cls(L)
        b5 = R[0, k][b]; b3 = R[1, k][b]
        a = np.zeros(L, dtype=np.float64)
        for l in range(1, min(m, L) + 1):
            if c[l]:
                p = np.float64(c[l]) * b3[l - 1:]
                a[:L - l + 1] = a[:L - l + 1] + p
        v = b5 * a
        N = np.float64(0.0)
        for x in sq.tile_sums(v):
            N = N + x
        out[t] = N / np.float64(M)
    return out


# ---- the checks of classes and bins

def check_positions(world, new):
    g = new(1000, 0)
    try:
        q = []
        T = world["lens"].size
        for t, L in enumerate(int(x) for x in world["lens"]):
            if L <= 129:
                q += [(t, p) for p in range(-2, L + 3)]
            else:
                q += [(t, p) for b in range(POS + 1) for p in (edge(b, L) - 1, edge(b, L), edge(b, L) + 1)]
        q += [(T, 5), (0xffffffff, 5), (T - 1, -2 ** 31), (T - 1, 2 ** 31 - 1)]
        tids, pos = (np.array(x) for x in zip(*q))
        got = g.position(tids.astype(np.uint32), pos)
        exp = probe(world, tids, pos)
        assert got.shape == exp.shape and np.array_equal(got, exp), np.flatnonzero((got != exp).any(axis=1))[:10]
        valid = exp[:, 0] >= 0
        assert valid.sum() > 1000 and (~valid).sum() > 40 and set(exp[valid, 0].tolist()) == set(range(CLASSES)) and set(exp[valid, 1].tolist()) == set(range(POS))
        # the edges are where the restatement says: B_b is the first position of bin b wherever the bin is not empty
        for t, L in enumerate(int(x) for x in world["lens"]):
            for b in range(POS):
                if edge(b, L) < edge(b + 1, L):
                    assert bin_of(edge(b, L), L) == b and bin_of(edge(b + 1, L) - 1, L) == b
        assert g.position([], []).size == 0
    finally:
        g.close()


# ---- the checks of the observed sweep

SIZES = (0, 1, 63, 64, 65, 255, 257, 5000)
fold_once = gc.fold_once


def assert_same(got_obs, got_stat, obs, st, what):
    got_obs = np.asarray(got_obs, dtype=np.uint64).reshape(SHAPE)
    assert np.array_equal(got_obs, obs), "%s: counts differ at %r" % (what, np.argwhere(got_obs != obs)[:5])
    assert {k: int(got_stat[k]) for k in STATS} == st, "%s: counters differ: %r, expected %r" % (what, {k: int(got_stat[k]) for k in STATS}, st)
    assert sum(int(got_stat[k]) for k in CATS) == int(got_stat["units"]), what


def check_against_restatement(world, new, off, hits, max_len=1000, max_blocks=0, what=""):
    c, s = fold_once(new, off, hits, max_len, max_blocks)
    eo, es = classify(world, off, hits, max_len)
    assert_same(c, s, eo, es, what)
    return eo, es


def check_sizes(world, new):
    for n in SIZES:
        off, h = gc.random_batch(world, n, 1000, seed=100 + n)
        eo, es = check_against_restatement(world, new, off, h, what="%d units" % n)
        if n == 5000:
            assert all(es[k] > 300 for k in CATS), es
            assert np.count_nonzero(eo) > 100


def check_grid_caps(world, new):
    off, h = gc.random_batch(world, 20001, 1000, seed=7)
    for mb in (1, 2, 0):
        check_against_restatement(world, new, off, h, max_blocks=mb, what="20 001 units, max_blocks %d" % mb)


def _one(tid, pos, mate_pos, frag_len):
    h = np.zeros(1, dtype=HIT_DTYPE)
    h["tid"] = tid; h["pos"] = pos; h["mate_pos"] = mate_pos; h["frag_len"] = frag_len; h["mate_status"] = 3; h["fwd"] = 1; h["mate_is_fwd"] = 0
    return h


def check_edges(world, new):
    """by hand: s and i on the edges of bins and one either side, a fragment that covers a whole transcript, e = L | L + 1, tid = n_txps,
    a fragment of one character, transcripts with empty bins"""
    lens = [int(x) for x in world["lens"]]; T = len(lens)
    for max_len in (1000, 40):
        rows = []                                                    # (record, category, (class, bin of s, bin of i) or None)
        for L in (1266, 5000, 129):
            t = lens.index(L); c = cls(L)
            for b in (1, 7, 19) if L > 129 else ():
                B = edge(b, L)
                f = min(30, max_len)
                rows += [(_one(t, B, B + 5, f), "used", (c, b, bin_of(B + f - 1, L))), (_one(t, B + 9, B - 1, f), "used", (c, b - 1, bin_of(B + f - 2, L))),
                         (_one(t, B - f + 1, B + 3, f), "used", (c, bin_of(B - f + 1, L), b)), (_one(t, B - f, B, f), "used", (c, bin_of(B - f, L), b - 1))]
            f = min(L, max_len)
            rows += [(_one(t, L - f, L, f), "used", (c, bin_of(L - f, L), 19)), (_one(t, L - f + 1, L, f), "overhang", None)]   # e = L | L + 1
            rows += [(_one(t, -4, 3, 5), "used", (c, 0, bin_of(4, L))), (_one(t, 10, 10, 1), "used", (c, bin_of(10, L), bin_of(10, L)))]
            rows += [(_one(t, 10, 10, max_len + 1), "out_of_range", None), (_one(t, 10, 10, 0), "out_of_range", None)]
        for L in (1, 2, 19, 20, 21, 40):                             # one fragment covers the whole transcript: bin 0 and the last position's
            if L <= max_len:
                rows += [(_one(lens.index(L), 0, 0, L), "used", (0, 0, bin_of(L - 1, L))), (_one(lens.index(L), 0, 0, L + 1), "overhang" if L + 1 <= max_len else "out_of_range", None)]
        rows += [(_one(lens.index(19), 7, 9, 5), "used", (0, bin_of(7, 19), bin_of(11, 19))), (_one(lens.index(791), 0, 0, 1), "used", (0, 0, 0)),
                 (_one(lens.index(792), 791, 791, 1), "used", (1, 19, 19)), (_one(lens.index(2433), 5, 5, 9), "used", (3, 0, 0)), (_one(lens.index(2434), 5, 5, 9), "used", (4, 0, 0)),
                 (_one(T, 10, 10, 5), "overhang", None), (_one(0xffffffff, 10, 10, 5), "overhang", None)]
        h = np.concatenate([r[0] for r in rows]); off = np.arange(len(rows) + 1, dtype=np.int64)
        for i, (rec, cat, where) in enumerate(rows):
            o1, s1 = classify(world, [0, 1], rec, max_len)
            assert s1[cat] == 1, (i, cat, s1)                        # the restatement agrees with the hand
            if where is not None:
                c, bs, bi = where
                assert o1[0, c, bs] == 1 and o1[1, c, bi] == 1, (i, where)
        eo, es = check_against_restatement(world, new, off, h, max_len=max_len, what="edges, max_len %d" % max_len)
        assert es["used"] == sum(1 for r in rows if r[1] == "used")


def check_one_bin(world, new):
    """the 64 lanes of one wavefront land in one bin (and 64 more in its neighbour): the slab's word takes them all"""
    lens = [int(x) for x in world["lens"]]
    t = lens.index(5000); B = edge(7, 5000)
    h = np.concatenate([_one(t, B + (i % 3), B + 40, 100) for i in range(64)] + [_one(t, B - 1, B + 40, 99) for i in range(64)])
    off = np.arange(129, dtype=np.int64)
    eo, es = check_against_restatement(world, new, off, h, what="one bin")
    assert es["used"] == 128 and eo[0, 4, 7] == 64 and eo[0, 4, 6] == 64 and eo[1, 4, bin_of(B + 99, 5000)] >= 64 and np.count_nonzero(eo) <= 5


def check_multi_units(world, new):
    rng = np.random.default_rng(11)
    cats = np.array([gc.MULTI, gc.U, gc.MULTI, gc.MULTI, gc.UNM, gc.MULTI, gc.U] * 3)
    for sizes in ((2,), (3,), (200,), (2, 3, 200)):
        off, h = gc.build(world, cats, 1000, rng, multi_sizes=sizes)
        eo, es = check_against_restatement(world, new, off, h, what="units of %r hits" % (sizes,))
        assert es["multi"] == 12 and es["unmapped"] == 3 and es["used"] == 6


def check_no_hits(world, new):
    for n in (1, 64, 300):
        off = np.zeros(n + 1, dtype=np.int64)
        for hits in (None, np.zeros(0, dtype=HIT_DTYPE)):
            c, s = fold_once(new, off, hits)
            assert not c.any() and s["unmapped"] == n == s["units"] and s["used"] == 0


def check_max_lens(world, new):
    for max_len in (1, 2, 1000, 1023):
        off, h = gc.random_batch(world, 700, max_len, seed=max_len)
        h["frag_len"][::5] = max_len + 1                             # just beyond, whatever the unit's category
        eo, es = check_against_restatement(world, new, off, h, max_len=max_len, what="max_len %d" % max_len)
        assert es["out_of_range"] > 20 and es["used"] > 5


def check_accumulate_and_clear(world, new):
    a = gc.random_batch(world, 3000, 1000, seed=21); b = gc.random_batch(world, 777, 1000, seed=22)
    ca, sa = classify(world, *a, 1000); cb, sb = classify(world, *b, 1000)
    f = new(1000, 2)
    try:
        f.add_hits(*a); f.add_hits(*b)
        assert_same(f.counts(), f.stat(), ca + cb, {k: sa[k] + sb[k] for k in STATS}, "two folds")
        assert f.stat()["folds"] == 2 and f.stat()["max_len"] == 1000
        f.clear()
        assert not f.counts().any() and all(f.stat()[k] == 0 for k in STATS)
        f.add_hits(*b)
        assert_same(f.counts(), f.stat(), cb, sb, "after clear")
    finally:
        f.close()


def check_add_counts(world, new):
    a = gc.random_batch(world, 3000, 1000, seed=31); b = gc.random_batch(world, 2049, 1000, seed=32)
    both = new(1000, 0); one = new(1000, 0); other = new(1000, 0)
    try:
        both.add_hits(*a); both.add_hits(*b)
        one.add_hits(*a); other.add_hits(*b)
        one.add_counts(other.counts())
        assert np.array_equal(one.counts(), both.counts())
        sb_, so = both.stat(), one.stat()
        # the counts bring their fragments only: the sum over end 0 goes to `used` and to the units, the other categories stay where they were swept
        _, sa = classify(world, *a, 1000); _, sbb = classify(world, *b, 1000)
        assert so["used"] == sb_["used"] == sa["used"] + sbb["used"] and sbb["used"] > 20
        assert so["units"] == sa["units"] + sbb["used"] and sum(so[k] for k in CATS) == so["units"]
        for k in CATS[1:]:
            assert so[k] == sa[k] and sb_[k] == sa[k] + sbb[k]
    finally:
        both.close(); one.close(); other.close()


OBS_CHECKS = {f.__name__[6:]: f for f in (check_sizes, check_grid_caps, check_edges, check_one_bin, check_multi_units, check_no_hits, check_max_lens,
                                          check_accumulate_and_clear, check_add_counts)}


# ---- the checks of the expected counts

EXPECT_NAMES = ("empty", "a single length", "every length 1..300", "sparse", "counts near 2^32", "1, L, L + 1, max_len at L = 20", "1, L, L + 1, max_len at L = 64",
                "1, L, L + 1, max_len at L = 792")


def weight_sets(world, counts):
    """name -> q uint64[T]: all ones; zeros; zeros but a few; one huge q_t that takes the bound to just below 2^63"""
    T = world["lens"].size; lens = [int(x) for x in world["lens"]]
    Pm = sq.prefix(counts)[-1]
    rng = np.random.default_rng(13)
    out = {"ones": np.ones(T, dtype=np.uint64), "zeros": np.zeros(T, dtype=np.uint64)}
    q = np.zeros(T, dtype=np.uint64); q[rng.integers(0, T, 4)] = rng.integers(1, 1000, 4).astype(np.uint64); out["sparse"] = q
    if Pm:
        q = np.ones(T, dtype=np.uint64); t = lens.index(1266)
        q[t] = np.uint64((2 ** 63 - 1 - (sum(lens) - lens[t]) * Pm) // (lens[t] * Pm))
        assert 2 ** 63 - lens[t] * Pm <= sq.weight_bound(q, lens, counts) < 2 ** 63
        out["one huge"] = q
    return out


def _check_expect(world, new, max_len, max_blocks, names=EXPECT_NAMES, sets=("ones", "zeros", "sparse", "one huge")):
    g = new(max_len, max_blocks)
    out = {}
    try:
        T = world["lens"].size
        for name, c in gc.histograms(world, max_len).items():
            if name not in names:
                continue
            for qn, q in weight_sets(world, c).items():
                if qn not in sets:
                    continue
                ex = g.expect(c, T, q)
                exp, total = expect(world, c, q)
                assert ex.dtype == np.uint64 and ex.shape == SHAPE
                assert np.array_equal(ex, exp), "%s, %s, max_len %d, max_blocks %d: differ at %r" % (name, qn, max_len, max_blocks, np.argwhere(ex != exp)[:5])
                assert_two_ends(ex, total, name)
                out[(name, qn)] = ex
        return out
    finally:
        g.close()


def check_expect_default_grid(world, new):
    got = _check_expect(world, new, 1000, 0)
    assert not got[("empty", "ones")].any() and not got[("sparse", "zeros")].any() and got[("every length 1..300", "ones")].all()
    assert max(int(v.max()) for v in got.values()) > 2 ** 55 and len(got) >= 25


def check_expect_max_len_1(world, new):
    _check_expect(world, new, 1, 0)


def check_expect_max_len_1023(world, new):
    _check_expect(world, new, 1023, 0, sets=("ones", "one huge"))


def check_expect_grid_caps(world, new):
    """one and two workgroups against the default grid: the same bits"""
    names = ("every length 1..300", "counts near 2^32")
    a = _check_expect(world, new, 1000, 0, names); b = _check_expect(world, new, 1000, 1, names); c = _check_expect(world, new, 1000, 2, names)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes()


def check_expect_twice_and_clear(world, new):
    g = new(1000, 0)
    try:
        T = world["lens"].size
        hs = gc.histograms(world, 1000)
        q = weight_sets(world, hs["sparse"])["sparse"]; ones = np.ones(T, dtype=np.uint64)
        a = g.expect(hs["sparse"], T, q)
        off, h = gc.random_batch(world, 300, 1000, seed=4)
        g.add_hits(off, h)
        g.clear()
        b = g.expect(hs["sparse"], T, q); c = g.expect(hs["every length 1..300"], T, ones); d = g.expect(hs["sparse"], T, q)
        assert a.tobytes() == b.tobytes() == d.tobytes() and np.array_equal(c, expect(world, hs["every length 1..300"], ones)[0])   # nothing is left over
        assert not g.counts().any()
    finally:
        g.close()


def check_expect_refusals(world, new):
    g = new(1000, 0)
    try:
        T = world["lens"].size; lens = [int(x) for x in world["lens"]]
        c = gc.histograms(world, 1000)["sparse"]
        q = weight_sets(world, c)["one huge"].copy()
        ex = g.expect(c, T, q)                                       # the largest that is taken
        assert_two_ends(ex, expect(world, c, q)[1], "just below the refusal")
        q[lens.index(1266)] += np.uint64(1)
        assert sq.weight_bound(q, lens, c) >= 2 ** 63
        try:
            g.expect(c, T, q)
        except Exception as e:
            assert "-4" in str(e), e
        else:
            raise AssertionError("a bound of 2^63 or more was accepted")
        big = np.full(T, 2 ** 64 - 1, dtype=np.uint64)               # (the sum over t does not wrap either)
        try:
            g.expect(c, T, big)
        except Exception as e:
            assert "-4" in str(e), e
        else:
            raise AssertionError("a bound beyond 2^64 was accepted")
        c0 = np.zeros(1001, dtype=np.uint64); c0[0] = 1
        for bad, n in ((c0, T), (np.zeros(1001, dtype=np.uint64), T + 1)):
            try:
                g.expect(bad, n, np.ones(n, dtype=np.uint64))
            except Exception as e:
                assert "-1" in str(e), e
            else:
                raise AssertionError("a bad argument was accepted")
    finally:
        g.close()


EXPECT_CHECKS = {f.__name__[6:]: f for f in (check_expect_default_grid, check_expect_max_len_1, check_expect_max_len_1023, check_expect_grid_caps,
                                             check_expect_twice_and_clear, check_expect_refusals)}


# ---- the host function; ratios_fn(obs, exp) is the implementation under test

def check_ratios(ratios_fn):
    rng = np.random.default_rng(81)
    obs = rng.integers(1, 100000, SHAPE).astype(np.uint64); ex = rng.integers(1, 1 << 50, SHAPE).astype(np.uint64)
    obs[0, 3, :] = 0                                                 # an (end, class) with no observations: all 1.0
    ex[1, 1, :] = 0                                                  # ... and one with nothing expected
    obs[0, 2, 0] = 10 ** 12; obs[0, 2, 1:] = 1; ex[0, 2, 0] = 0; ex[0, 2, 1:] = 10 ** 6      # the upper clamp
    obs[1, 4, 19] = 0; obs[1, 4, :19] = 10 ** 9; ex[1, 4, :] = 1000                          # the lower clamp
    obs[1, 0, 5] = 0; ex[0, 0, 7] = 0                                # single zeros inside rows that have counts
    R = ratios_fn(obs, ex); E = ratios(obs, ex)
    assert R.dtype == np.float64 and R.shape == SHAPE and R.tobytes() == E.tobytes()
    assert (R[0, 3] == 1.0).all() and (R[1, 1] == 1.0).all() and R.min() == 0.25 and R.max() == 4.0
    assert R[0, 2, 0] == 4.0 and R[1, 4, 19] == 0.25 and (R[1, 0] != 1.0).all() and len(set(R.ravel().tolist())) > 50
    z = np.zeros(SHAPE, dtype=np.uint64)
    assert (ratios_fn(z, z) == 1.0).all() and (ratios_fn(obs, z) == 1.0).all() and (ratios_fn(z, ex) == 1.0).all()


# ---- the checks of the effective lengths

eff_histograms = sq.eff_histograms


def random_ratios(seed):
    rng = np.random.default_rng(seed)
    return np.exp2(rng.uniform(-2, 2, SHAPE))


def check_eff_ratio_one(world, new, fld_fn=None):
    """(a) R == 1: the fragment-length model's effective length as one quotient, bit for bit"""
    g = new(1000, 0)
    try:
        T = world["lens"].size
        for name, c in eff_histograms().items():
            e = g.eff_lens(c, T, np.ones(SHAPE))
            assert e.tobytes() == sq.fld_quotient(world, c).tobytes(), name
            if fld_fn is not None:
                assert np.allclose(e, fld_fn(c, world["lens"]), rtol=1e-12, atol=0)   # (L + 1) - Q / P: the same number by another formula
    finally:
        g.close()


def check_eff_powers_of_two(world, new):
    """(b) R = 2^a on all of end 0 and 2^b on all of end 1: 2^(a + b) times the quotient of (a), bit for bit (a power of two scales every
    term and every partial sum exactly)"""
    T = world["lens"].size
    g = new(1000, 0)
    try:
        for a, b in ((1, 0), (-2, 2), (2, 2), (-2, -2), (0, -1)):
            R = np.ones(SHAPE); R[0] = 2.0 ** a; R[1] = 2.0 ** b
            for name, c in eff_histograms().items():
                e = g.eff_lens(c, T, R)
                base = sq.fld_quotient(world, c)
                P = sq.prefix(c); fits = np.array([P[min(int(L), 1000)] > 0 for L in world["lens"]])
                exp = np.where(fits, base * np.float64(2.0 ** (a + b)), base)   # (where no fragment fits: L_t, whatever R)
                assert e.tobytes() == exp.tobytes(), (a, b, name)
    finally:
        g.close()


def check_eff_random(world, new):
    """(c) random R in [0.25, 4]: the restatement that spells out the tree, bit for bit; max_len 1000, 1023 and 100"""
    T = world["lens"].size
    for max_len in (1000, 1023, 100):
        g = new(max_len, 0)
        try:
            for i, (name, c) in enumerate(eff_histograms(max_len).items()):
                R = random_ratios(93 + i)
                e = g.eff_lens(c, T, R)
                assert e.tobytes() == eff_lens(world["lens"], c, R).tobytes(), (max_len, name)
                assert (e != sq.fld_quotient(world, c)).sum() > 3
        finally:
            g.close()


def check_eff_grid_caps(world, new):
    """(d) one and two workgroups against the default grid, bit for bit (a run of tiles then starts in the middle of a transcript)"""
    c = eff_histograms()["a run's"]; R = random_ratios(95); T = world["lens"].size
    out = []
    for mb in (0, 1, 2):
        g = new(1000, mb)
        try:
            out.append(g.eff_lens(c, T, R)); out.append(g.eff_lens(c, T, R))
        finally:
            g.close()
    assert all(o.tobytes() == out[0].tobytes() for o in out) and out[0].tobytes() == eff_lens(world["lens"], c, R).tobytes()


def check_eff_short_transcripts(world, new):
    """(e) a transcript shorter than every length with counts -> L_t"""
    c = np.zeros(1001, dtype=np.uint64); c[500] = 4; c[900] = 1
    g = new(1000, 0)
    try:
        e = g.eff_lens(c, world["lens"].size, random_ratios(96))
        try:
            bad = c.copy(); bad[0] = 1
            g.eff_lens(bad, world["lens"].size, np.ones(SHAPE))
        except Exception as ex:
            assert "-1" in str(ex), ex
        else:
            raise AssertionError("counts[0] != 0 was accepted")
    finally:
        g.close()
    lens = world["lens"]
    assert np.array_equal(e[lens < 500], lens[lens < 500].astype(np.float64)) and (lens < 500).sum() >= 10
    assert e.tobytes() == eff_lens(lens, c, random_ratios(96)).tobytes()


EFF_CHECKS = {f.__name__[10:]: f for f in (check_eff_ratio_one, check_eff_powers_of_two, check_eff_random, check_eff_grid_caps, check_eff_short_transcripts)}


def write_fasta(path, seqs):
    with open(path, "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b">t%d\n" % i + s + b"\n")


# ---- the planted bias: fragments thinned by where on their transcript they start

PLANTED_SEED = 277
PLANTED_DRAWS = 24000
PLANTED_KEEP = (0.2, 1.0)                                            # the probability to keep a fragment: linear in s / L from the first to the second
PLANTED_GENES = 12
PLANTED_SHARED, PLANTED_OWN_A, PLANTED_OWN_B = 500, 300, 1500        # a gene: isoform A = own (300) + shared (500), isoform B = shared (500) + own (1500)


def planted_transcripts(seed=PLANTED_SEED):
    """-> (names, transcripts uint8, abundances).  Decoy transcripts of their own, six of each of five lengths, one length per class
    (700, 1100, 1500, 2000, 2800): they map uniquely, so what is observed along them shows the bias per class whatever their
    abundances.  PLANTED_GENES genes of two isoforms that share a stretch of PLANTED_SHARED characters: it lies at the 3' end of the
    short isoform A (800 characters, class 1) and at the 5' end of the long isoform B (2 000 characters, class 3).  A fragment of
    the shared stretch maps to both isoforms; how the estimate splits those is what the effective lengths decide.  The two isoforms
    differ in length, so the same relative thinning costs them different shares of their fragments: a bias that is the same for
    every transcript of a gene would be absorbed by the first estimate and show nothing."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    rs = lambda n: acgt[rng.integers(0, 4, n)]
    names, txps = [], []
    for L in (700, 1100, 1500, 2000, 2800):
        for i in range(6):
            names.append("S%d.%d" % (L, i)); txps.append(rs(L))
    for gene in range(PLANTED_GENES):
        shared = rs(PLANTED_SHARED)
        names.append("G%d.A" % gene); txps.append(np.concatenate([rs(PLANTED_OWN_A), shared]))
        names.append("G%d.B" % gene); txps.append(np.concatenate([shared, rs(PLANTED_OWN_B)]))
    theta = rng.uniform(0.5, 2.0, len(txps))
    return names, txps, theta


def planted_draws(txps, theta, n_draws=PLANTED_DRAWS, seed=PLANTED_SEED + 1):
    """the kept fragments as (tid, start, length) int64 arrays: a transcript by abundance x length, a length of N(220, 20) clipped to
    [150, 300], a start uniform over the transcript; each kept with a probability linear in start / L between PLANTED_KEEP's two"""
    rng = np.random.default_rng(seed)
    lens = np.array([t.size for t in txps], dtype=np.int64)
    w = theta * lens
    tid = rng.choice(len(txps), size=n_draws, p=w / w.sum())
    flen = np.clip(rng.normal(220, 20, n_draws).astype(np.int64), 150, 300)
    start = (rng.random(n_draws) * (lens[tid] - flen + 1)).astype(np.int64)
    keep = rng.random(n_draws) < PLANTED_KEEP[0] + (PLANTED_KEEP[1] - PLANTED_KEEP[0]) * start / lens[tid]
    return tid[keep], start[keep], flen[keep]


def planted_fragments(txps, theta, n_draws=PLANTED_DRAWS, seed=PLANTED_SEED + 1, read_len=60):
    """-> (reads1, reads2 as lists of bytes, mate 2 reverse-complemented, the mates swapped in half of the pairs; tid int64[kept] of the
    transcript each kept fragment came from)"""
    from rapmap_amd.synth import _COMP
    tid, start, flen = planted_draws(txps, theta, n_draws, seed)
    swap = np.random.default_rng(seed + 7).random(tid.size) < 0.5
    r1, r2 = [], []
    for i in range(tid.size):
        f = txps[int(tid[i])][int(start[i]):int(start[i] + flen[i])]
        a = f[:read_len].tobytes(); b = _COMP[f[::-1][:read_len]].tobytes()
        if swap[i]:
            a, b = b, a
        r1.append(a); r2.append(b)
    return r1, r2, tid
