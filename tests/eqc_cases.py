"""Inputs and expected answers of the equivalence-class tests (test_eq_classes.py: lane emulation, test_eq_classes_gpu.py: device).
The expected table of a set of lists is a dictionary built here: tuple(sorted(set(tids))) -> count, in canonical order."""
import numpy as np

BIG = (1 << 31) + 5          # a tid beyond 2^31: compares must be unsigned
LENGTHS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 201, 1000, 1100]   # across a group (8), a wavefront (64), the LDS slab (2048 with repeats below)


def crafted_lists(seed=7, n_fill=2900):
    """(lists, weights): about 3 000 lists -- every shape the label stage has a path for, then a skewed random fill so that several
    wavefronts contend for the same few slots"""
    rng = np.random.default_rng(seed)
    L = [[], [7], [5, 5, 5], [3, 9, 20, 1, 9, 30], [90, 80, 70, 60, 50, 40, 30, 20, 10], [], [0], [BIG], [0, BIG], [BIG, 0, BIG, 0],
         [1, 2, 3, 4], [1, 2, 3],                                   # a label and its proper prefix
         [10, 20, 30], [30, 10, 20, 10], [20, 20, 30, 30, 10, 10, 20]]   # one label, three orders, different repeats
    for n in LENGTHS:
        base = rng.choice(5000, size=n, replace=False).astype(np.int64) * 3 + 11
        L.append(list(base))                                        # n distinct tids, random order
        L.append(list(base[::-1]))                                  # ... the same label again, another order
        if n > 1:
            L.append(list(np.concatenate([np.sort(base[: n // 2]), np.sort(base[n // 3:])])))   # two ascending runs that overlap: repeats
    L.append(list(np.arange(2500, 0, -1)))                          # descending, beyond the slab: sorted in place in device memory
    L.append(list(rng.integers(0, 40, size=2300)))                  # beyond the slab, mostly repeats
    hot = [[4], [4, 8], [2, 4, 8], [100, 200, 300, 400, 500, 600, 700, 800, 900]]
    for i in range(n_fill):
        r = rng.random()
        if r < 0.5:
            L.append(list(rng.permutation(hot[int(rng.integers(0, 4))])))
        elif r < 0.55:
            L.append([])
        else:
            k = int(rng.integers(1, 12))
            L.append(list(rng.integers(0, 30, size=k)))
    order = rng.permutation(len(L))
    L = [L[i] for i in order]
    w = rng.integers(1, 1000, size=len(L)).astype(np.uint64)
    w[::17] = (1 << 40) + 3                                          # sums beyond 32 bits
    return L, w


def distinct_labels(n, seed=3, width=3):
    """n lists with n different labels (list i holds i and width - 1 random tids above n)"""
    rng = np.random.default_rng(seed)
    return [[i] + list(rng.integers(n, 2 * n, size=width - 1)) for i in range(n)]


def csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    if lists:
        np.cumsum([len(x) for x in lists], out=off[1:])
    tids = np.array([t for x in lists for t in x], dtype=np.uint32)
    return off, tids


def expected(lists, weights=None):
    d = {}
    for i, x in enumerate(lists):
        if len(x):
            k = tuple(sorted(set(int(t) for t in x)))
            d[k] = d.get(k, 0) + (1 if weights is None else int(weights[i]))
    return d


def expected_from_hits(hit_offsets, hits):
    tid = np.asarray(hits["tid"]); ho = np.asarray(hit_offsets)
    return expected([tid[ho[i]:ho[i + 1]] for i in range(len(ho) - 1)])


def canonical(d):
    """the dictionary as the three arrays a fetch returns: labels ascending (tuples compare the way the table orders them)"""
    keys = sorted(d)
    off = np.zeros(len(keys) + 1, dtype=np.int64)
    if keys:
        np.cumsum([len(k) for k in keys], out=off[1:])
    return off, np.array([t for k in keys for t in k], dtype=np.uint32), np.array([d[k] for k in keys], dtype=np.uint64)


def assert_table(got, d, what=""):
    off, tids, cnt = canonical(d)
    g_off, g_tids, g_cnt = got
    assert np.array_equal(np.asarray(g_off, dtype=np.int64), off), "%s: label offsets differ (%d classes, %d expected)" % (what, len(g_off) - 1, len(off) - 1)
    assert np.array_equal(np.asarray(g_tids, dtype=np.uint32), tids), "%s: labels differ" % what
    assert np.array_equal(np.asarray(g_cnt, dtype=np.uint64), cnt), "%s: counts differ" % what
