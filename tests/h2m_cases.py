"""Inputs and expected answers of the hits-to-mappings tests of the lean kernel (test_h2m_tiles.py: lane emulation, test_h2m_tiles_gpu.py: device).

The pass (qm_lean.inl) has four editions -- the dispatcher the kernels call (lean_h2m), the scalar-indexed loop (lean_h2m_loop), the 8 x 8 tiles
(lean_h2m_tiles, n <= 32) and their single-tile edition (n <= 8) -- held against one another and against a plain restatement of the rule:

  * a transcript survives when it was seen in every one of the m intervals;
  * it is represented by its entry with the smallest (position, order of the interval -- the first smallest interval first, then the
    others in their own order --, lane);
  * `slot` of a lane is the number of survivors with a smaller transcript id, `elem` its (transcript, strand, position - queryPos),
    and the return value is the number of survivors.

Every test body is a function of `h2m_many(which, cases)`: cases = [(stash (n, 4) rows {tid, pos, qp, iv}, m, min_idx, is_rc)] -> for every case
(count, elem[64], keep[64], slot[64]).  A body collects its cases and runs each edition once over those it takes."""
import numpy as np

DISPATCH, LOOP, TILES, ONE_TILE = 0, 1, 2, 3                      # `which`
EDITIONS = (("lean_h2m", DISPATCH, 64), ("lean_h2m_loop", LOOP, 64), ("lean_h2m_tiles", TILES, 32), ("lean_h2m_tiles<ONE>", ONE_TILE, 8))   # (name, which, largest n)


def rule(stash, m, min_idx, is_rc):
    """the rule, entry by entry -> (count, elem[n], keep[n], slot[n])"""
    st = [tuple(int(x) for x in r) for r in np.asarray(stash, dtype=np.uint32).reshape(-1, 4)]
    n = len(st)

    def order(iv):
        return 0 if iv == min_idx else (iv + 1 if iv < min_idx else iv)

    by_tid = {}
    for l, (t, ps, qp, iv) in enumerate(st):
        by_tid.setdefault(t, []).append(l)
    keep = [False] * n
    for t, lanes in by_tid.items():
        if {st[l][3] for l in lanes} == set(range(m)):
            keep[min(lanes, key=lambda l: (st[l][1], order(st[l][3]), l))] = True
    alive = sorted(st[l][0] for l in range(n) if keep[l])
    slot = [int(np.searchsorted(alive, st[l][0], side="left")) for l in range(n)]
    elem = [(t << 33) | ((1 if is_rc else 0) << 32) | ((ps - qp) & 0xffffffff) for (t, ps, qp, iv) in st]
    return len(alive), elem, keep, slot


def check_all(h2m_many, cases):
    """every edition that takes a case's n, once over all such cases, against the rule"""
    cases = [(np.asarray(st, dtype=np.uint32).reshape(-1, 4), m, mi, rc) for st, m, mi, rc in cases]
    wants = [rule(*c) for c in cases]
    for name, which, nmax in EDITIONS:
        idx = [i for i, c in enumerate(cases) if len(c[0]) <= nmax]
        if not idx:
            continue
        got = h2m_many(which, [cases[i] for i in idx])
        assert len(got) == len(idx)
        for i, (cnt, elem, keep, slot) in zip(idx, got):
            stash, m, min_idx, _ = cases[i]
            n = len(stash); want = wants[i]
            ctx = "%s: n %d, m %d, minIdx %d\n%s" % (name, n, m, min_idx, stash)
            assert cnt == want[0], ctx
            assert [bool(x) for x in keep[:n]] == want[2], ctx
            assert not keep[n:].any(), ctx                                # lanes n .. keep nothing
            assert [int(x) for x in elem[:n]] == want[1], ctx
            assert [int(x) for x in slot[:n]] == want[3], ctx


def by_interval(rows):
    """the order the walks leave: one interval's suffixes after the other"""
    return sorted(rows, key=lambda r: r[3])                          # (stable)


TIDS = (0, 1, 2, 5, 77, 1000, 65535, 65536, 0x7ffffffe, 0x7fffffff)


def random_stash(rng, n, m):
    """n entries over m intervals, about half of them from transcripts that sit in every interval"""
    pool = [int(t) for t in rng.permutation(np.concatenate([np.array(TIDS), rng.integers(0, 1 << 31, 64)]))]
    rows = []
    full = 0 if m > n else int(rng.integers(0, n // m + 1))            # transcripts present in all m intervals
    qps = [int(q) for q in np.sort(rng.integers(0, 100, m))]
    npos = int(rng.choice([1, 2, 4, 1000]))
    for t in pool[:full]:
        for iv in range(m):
            rows.append((t, int(rng.integers(0, npos)) + 200, qps[iv], iv))
    extra = pool[: full + 1 + int(rng.integers(0, 4))]                # more of the same transcripts (twice in an interval) and a few partial ones
    while len(rows) < n:
        iv = int(rng.integers(0, m))
        rows.append((extra[int(rng.integers(0, len(extra)))], int(rng.integers(0, npos)) + 200, qps[iv], iv))
    rows = rows[:n]
    return by_interval(rows) if rng.integers(0, 4) else [rows[i] for i in rng.permutation(len(rows))] if rows else rows


RANDOM_NS = range(0, 65)


def random_stashes(h2m_many, n):
    rng = np.random.default_rng(1000 + n)
    ms = sorted(set([1, 2, 32] + [int(x) for x in rng.integers(1, 33, 8)] + [(n % 32) + 1, ((n * 7) % 32) + 1]))
    cases = []
    for m in ms:
        for rep in range(5):
            stash = random_stash(rng, n, m)
            cases.append((stash, m, int(rng.integers(0, m)), bool(rep & 1)))
    check_all(h2m_many, cases)


def every_interval_count(h2m_many):
    """m = 1 .. 32 with a transcript in every interval and one that misses the last"""
    cases = []
    for m in range(1, 33):
        rows = [(9, 300 + iv, iv, iv) for iv in range(m)] + [(4, 100, iv, iv) for iv in range(m - 1)]
        for mi in (0, m // 2, m - 1):
            cases.append((by_interval(rows), m, mi, False))
    check_all(h2m_many, cases)


SIZES = (8, 9, 16, 17, 32, 33, 64)


def one_transcript_fills_the_stash(h2m_many, n):
    """all n entries of one transcript: one survivor, the smallest position (the first of them on ties)"""
    cases = []
    for m in (1, 2, 3):
        rows = by_interval([(42, 500 - (i % 5), 3 * (i % m), i % m) for i in range(n)])
        for mi in range(m):
            cases.append((rows, m, mi, False))
        cases.append(([(42, 7, 0, i * m // n) for i in range(n)], m, m - 1, False))          # every position equal
    check_all(h2m_many, cases)


def twice_in_one_interval(h2m_many, n):
    """every transcript twice in interval 0 and once in interval 1"""
    t = n // 3
    rows = [(10 + i, 100 + i, 0, 0) for i in range(t)] + [(10 + i, 90 + (i % 3), 0, 0) for i in range(t)] + [(10 + i, 95, 20, 1) for i in range(t)]
    rows += [(5, 1, 0, 1)] * (n - 3 * t)                                        # (fill: a transcript of interval 1 only)
    check_all(h2m_many, [(by_interval(rows), 2, mi, False) for mi in (0, 1)])


def missing_from_one_interval(h2m_many, n):
    """three intervals; every third transcript misses one of them, which one rotating"""
    rows = []
    t = 0
    while len(rows) + 3 <= n:
        miss = (t // 3) % 3 if t % 3 == 0 else -1
        rows += [(1000 - t, 50 + t, 10 * iv, iv) for iv in range(3) if iv != miss]
        t += 1
    rows += [(2000, 1, 0, 2)] * (n - len(rows))
    check_all(h2m_many, [(by_interval(rows), 3, mi, False) for mi in range(3)])


def equal_positions_min_idx_decides(h2m_many, n):
    """every transcript at one position in all m intervals: its entry of interval minIdx represents it (first, middle and last)"""
    cases = []
    for m in (2, 3, 4, 8):
        t = n // m
        rows = [(300 + 2 * i, 1234, 7 * iv, iv) for iv in range(m) for i in range(t)]
        rows += [(299, 1234, 0, 0)] * (n - t * m)
        for mi in (0, m // 2, m - 1):
            cases.append((by_interval(rows), m, mi, False))
            cases.append((by_interval(rows), m, mi, True))
    check_all(h2m_many, cases)


def thresholds_of_the_dispatcher(h2m_many, tile_range):
    """the sizes at which lean_h2m changes edition, one below and one above each"""
    lo, hi = tile_range
    assert 0 <= lo <= hi <= 32
    rng = np.random.default_rng(7)
    cases = []
    for n in sorted({max(lo - 1, 0), lo, lo + 1, 7, 8, 9, hi - 1, hi, hi + 1}):
        for m in (1, 2, 3):
            for _ in range(20):
                cases.append((random_stash(rng, n, m), m, int(rng.integers(0, m)), False))
    check_all(h2m_many, cases)
