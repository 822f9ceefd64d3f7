"""Inputs, the restatement and the checks of the fragment-length tests (test_fld.py: lane emulation and the host arithmetic,
test_fld_gpu.py: device).  Everything here is exact: integer counts, and effective lengths compared bit for bit.

classify() restates the six categories of include/qmap_mi355.h in numpy; eff_lens() restates the arithmetic in float64 with its two
operations spelled out.  A check takes `new(max_len, max_blocks)`, which makes a histogram object with add_hits / add_counts /
counts / stat / clear / close -- rapmap_amd.FragLenDist on the device, emu_fld.EmuFld under the lane emulation."""
import numpy as np

from rapmap_amd.api import HIT_DTYPE

CATS = ("used", "unmapped", "multi", "not_paired", "same_strand", "out_of_range")
STATS = ("units",) + CATS
U, UNM, MULTI, NP, SS, OOR = range(6)


def classify(hit_offsets, hits, max_len):
    """-> (counts uint64[max_len + 1], stats): every unit in the first category whose condition holds"""
    off = np.asarray(hit_offsets, dtype=np.int64)
    n = len(off) - 1
    cnt = np.diff(off)
    st = dict.fromkeys(STATS, 0)
    st["units"] = n
    st["unmapped"] = int(np.count_nonzero(cnt == 0))
    st["multi"] = int(np.count_nonzero(cnt >= 2))
    counts = np.zeros(max_len + 1, dtype=np.uint64)
    one = off[:-1][cnt == 1]
    if one.size:
        h = np.asarray(hits)[one]
        fl = h["frag_len"].astype(np.uint64)                        # unsigned 32-bit numbers
        not_paired = h["mate_status"] != 3
        same = ~not_paired & (h["fwd"] == h["mate_is_fwd"])
        oor = ~not_paired & ~same & ((fl == 0) | (fl > max_len))
        used = ~not_paired & ~same & ~oor
        st["not_paired"] = int(not_paired.sum()); st["same_strand"] = int(same.sum()); st["out_of_range"] = int(oor.sum()); st["used"] = int(used.sum())
        counts += np.bincount(fl[used].astype(np.int64), minlength=max_len + 1).astype(np.uint64)
    assert sum(st[k] for k in CATS) == n and counts[0] == 0 and int(counts.sum()) == st["used"]
    return counts, st


def eff_lens(counts, lens):
    """float64[len(lens)]: L when no fragment length fits, else (double)(L + 1) - (double)Q[m] / (double)P[m], m = min(L, max_len)"""
    c = [int(x) for x in counts]
    max_len = len(c) - 1
    P = [0] * (max_len + 1); Q = [0] * (max_len + 1)
    for l in range(1, max_len + 1):
        P[l] = P[l - 1] + c[l]; Q[l] = Q[l - 1] + l * c[l]
    assert Q[max_len] < 2 ** 53
    out = np.zeros(len(lens), dtype=np.float64)
    for i, L in enumerate(int(x) for x in lens):
        m = min(L, max_len)
        if P[m] == 0:
            out[i] = np.float64(L)
        else:
            mean = np.float64(Q[m]) / np.float64(P[m])              # one division
            out[i] = np.float64(L + 1) - mean                       # one subtraction
    return out


# ---- case builders

def _records(rng, n):
    """n hit records of random bytes in every field the sweep must not look at"""
    h = np.zeros(n, dtype=HIT_DTYPE)
    h["tid"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    h["pos"] = rng.integers(-50, 1 << 20, n); h["mate_pos"] = rng.integers(-50, 1 << 20, n)
    h["read_len"] = rng.integers(0, 300, n); h["mate_len"] = rng.integers(0, 300, n)
    h["is_paired"] = rng.integers(0, 2, n); h["aln_score"] = rng.integers(-100, 100, n)
    return h


def build(cats, max_len, rng, frag_lens=None, multi_sizes=(2, 3)):
    """units of the given categories -> (hit_offsets, hits).  The first record of every unit with hits would qualify as `used` if
    it stood alone and unchanged, except for the one field its category turns"""
    cats = np.asarray(cats, dtype=np.int64)
    n = cats.size
    k = np.ones(n, dtype=np.int64)
    k[cats == UNM] = 0
    nm = int(np.count_nonzero(cats == MULTI))
    if nm:
        k[cats == MULTI] = rng.choice(np.asarray(multi_sizes), size=nm)
    off = np.zeros(n + 1, dtype=np.int64); np.cumsum(k, out=off[1:])
    h = _records(rng, int(off[-1]))
    # every record: properly paired, opposite strands, a length in range
    h["mate_status"] = 3
    h["fwd"] = rng.integers(0, 2, h.size); h["mate_is_fwd"] = 1 - h["fwd"]
    h["frag_len"] = rng.integers(1, max_len + 1, h.size)
    first = off[:-1]
    if frag_lens is not None:
        sel = cats == U
        h["frag_len"][first[sel]] = np.asarray(frag_lens, dtype=np.uint32)[: int(sel.sum())]
    i = first[cats == NP]
    h["mate_status"][i] = rng.integers(0, 3, i.size)
    i = first[cats == SS]
    h["mate_is_fwd"][i] = h["fwd"][i]
    i = first[cats == OOR]
    h["frag_len"][i] = rng.choice(np.array([0, max_len + 1, 0x7fffffff, 0xffffffff, max_len + 7], dtype=np.uint32), size=i.size)
    return off, h


def random_batch(n, max_len, seed, every_wave=True):
    """n units of random categories; with every_wave the first six units of every 64 hold the six categories"""
    rng = np.random.default_rng(seed)
    cats = rng.integers(0, 6, n)
    if every_wave:
        for b in range(0, n - 5, 64):
            cats[b:b + 6] = rng.permutation(6)
    return build(cats, max_len, rng)


def fold_once(new, off, hits, max_len=1000, max_blocks=0):
    f = new(max_len, max_blocks)
    try:
        f.add_hits(off, hits)
        return f.counts(), f.stat()
    finally:
        f.close()


def assert_same(got_counts, got_stat, counts, st, what):
    assert np.array_equal(np.asarray(got_counts, dtype=np.uint64), counts), "%s: bins differ" % what
    assert {k: int(got_stat[k]) for k in STATS} == st, "%s: counters differ: %r, expected %r" % (what, {k: int(got_stat[k]) for k in STATS}, st)
    assert sum(int(got_stat[k]) for k in CATS) == int(got_stat["units"]), what


def check_against_restatement(new, off, hits, max_len=1000, max_blocks=0, what=""):
    c, s = fold_once(new, off, hits, max_len, max_blocks)
    ec, es = classify(off, hits, max_len)
    assert_same(c, s, ec, es, what)
    return ec, es


# ---- the crafted checks, by name; each the smallest shape at which that part of the kernel can still go wrong

SIZES = (0, 1, 63, 64, 65, 255, 257, 5000)


def check_sizes(new):
    for n in SIZES:
        off, h = random_batch(n, 1000, seed=100 + n)
        ec, es = check_against_restatement(new, off, h, what="%d units" % n)
        if n == 5000:                                                # every category present in every wavefront
            cnt = np.diff(off)
            for b in range(0, n - 63, 64):
                _, sb = classify(off[b:b + 65] - off[b], h[off[b]:off[b + 64]], 1000)
                assert all(sb[k] > 0 for k in CATS), (b, sb)
            assert cnt.max() == 3 and es["used"] > 500


def _check_ragged(new, max_blocks):
    off, h = random_batch(70001, 1000, seed=7)
    check_against_restatement(new, off, h, max_blocks=max_blocks, what="70 001 units, max_blocks %d" % max_blocks)


def check_ragged_one_block(new):
    _check_ragged(new, 1)


def check_ragged_two_blocks(new):
    _check_ragged(new, 2)


def check_ragged_default_grid(new):
    _check_ragged(new, 0)


def check_frag_len_edges(new):
    for max_len in (1000, 2):
        rng = np.random.default_rng(5)
        vals = np.array([0, 1, max_len, max_len + 1, 0x7fffffff, 0xffffffff], dtype=np.uint32)
        off, h = build(np.full(6, U), max_len, rng, frag_lens=vals)
        c, s = fold_once(new, off, h, max_len)
        exp = np.zeros(max_len + 1, dtype=np.uint64); exp[1] += 1; exp[max_len] += 1
        assert np.array_equal(c, exp)
        assert (s["used"], s["out_of_range"], s["units"]) == (2, 4, 6)
        ec, es = classify(off, h, max_len)
        assert_same(c, s, ec, es, "frag_len edges, max_len %d" % max_len)


def check_multi_units(new):
    rng = np.random.default_rng(11)
    cats = np.array([MULTI, U, MULTI, MULTI, UNM, MULTI, U] * 3)
    for sizes in ((2,), (3,), (200,), (2, 3, 200)):
        off, h = build(cats, 1000, rng, multi_sizes=sizes)
        first = off[:-1][np.diff(off) >= 2]
        _, alone = classify(np.arange(first.size + 1), h[first], 1000)
        assert alone["used"] == first.size                           # every first record would qualify if it were alone
        ec, es = check_against_restatement(new, off, h, what="units of %r hits" % (sizes,))
        assert es["multi"] == 12 and es["used"] == 6


def check_hot_bin(new):
    rng = np.random.default_rng(13)
    off, h = build(np.full(5000, U), 1000, rng, frag_lens=np.full(5000, 311))
    c, s = fold_once(new, off, h)
    assert int(c[311]) == 5000 and int(c.sum()) == 5000 and s["used"] == 5000 and s["units"] == 5000


def check_every_bin(new):
    for max_len in (1000, 1023):
        rng = np.random.default_rng(17)
        off, h = build(np.full(max_len, U), max_len, rng, frag_lens=rng.permutation(max_len) + 1)
        c, s = fold_once(new, off, h, max_len)
        exp = np.ones(max_len + 1, dtype=np.uint64); exp[0] = 0
        assert np.array_equal(c, exp) and s["used"] == max_len      # ... the last word of the slab at 1023


def check_no_hits(new):
    for n in (1, 64, 300):
        off = np.zeros(n + 1, dtype=np.int64)
        for hits in (None, np.zeros(0, dtype=HIT_DTYPE)):
            c, s = fold_once(new, off, hits)
            assert not c.any() and s["unmapped"] == n == s["units"] and s["used"] == 0


def check_max_lens(new):
    for max_len in (1, 2, 1000, 1023):
        off, h = random_batch(700, max_len, seed=max_len)
        h["frag_len"][::5] = max_len + 1                             # just beyond, whatever the unit's category
        ec, es = check_against_restatement(new, off, h, max_len=max_len, what="max_len %d" % max_len)
        assert es["used"] > 50 and es["out_of_range"] > 20


def check_accumulate_and_clear(new):
    a = random_batch(3000, 1000, seed=21); b = random_batch(777, 1000, seed=22)
    ca, sa = classify(*a, 1000); cb, sb = classify(*b, 1000)
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


def check_add_counts(new):
    a = random_batch(3000, 1000, seed=31); b = random_batch(2049, 1000, seed=32)
    both = new(1000, 0); one = new(1000, 0); other = new(1000, 0)
    try:
        both.add_hits(*a); both.add_hits(*b)
        one.add_hits(*a); other.add_hits(*b)
        one.add_counts(other.counts())
        assert np.array_equal(one.counts(), both.counts())
        sb_, so = both.stat(), one.stat()
        # the counts bring their fragments only: `used` and the units grow by their sum, the other categories stay where they were folded
        _, sa = classify(*a, 1000); cb, sbb = classify(*b, 1000)
        assert so["used"] == sb_["used"] == sa["used"] + sbb["used"]
        assert so["units"] == sa["units"] + sbb["used"] and sum(so[k] for k in CATS) == so["units"]
        for k in CATS[1:]:
            assert so[k] == sa[k] and sb_[k] == sa[k] + sbb[k]
        bad = np.zeros(1001, dtype=np.uint64); bad[0] = 1
        try:
            one.add_counts(bad)
        except Exception as e:
            assert "-1" in str(e)                                    # QM_E_ARG
        else:
            raise AssertionError("counts[0] != 0 was accepted")
    finally:
        both.close(); one.close(); other.close()


CHECKS = {f.__name__[6:]: f for f in (check_sizes, check_ragged_one_block, check_ragged_two_blocks, check_ragged_default_grid, check_frag_len_edges,
                                      check_multi_units, check_hot_bin, check_every_bin, check_no_hits, check_max_lens, check_accumulate_and_clear,
                                      check_add_counts)}


# ---- effective lengths; `fn(counts, lens)` is the implementation under test, `Err` what it raises with the status in its text

def eff_check_lengths(fn, Err):
    max_len = 1000
    rng = np.random.default_rng(41)
    c = np.zeros(max_len + 1, dtype=np.uint64)
    c[180:420] = rng.integers(0, 5000, 240).astype(np.uint64); c[180] = 3; c[999] = 1
    shortest = 180
    lens = np.array([1, shortest - 1, shortest, max_len, max_len + 1, 10 ** 5, 2 ** 32 - 1], dtype=np.uint64)
    got = fn(c, lens); exp = eff_lens(c, lens)
    assert got.dtype == np.float64 and got.tobytes() == exp.tobytes(), (got, exp)
    assert got[0] == 1.0 and got[1] == shortest - 1 and got[2] == 1.0 and got[-1] < 2 ** 32


def eff_check_empty(fn, Err):
    lens = np.array([1, 2, 999, 1000, 1001, 10 ** 5, 2 ** 32 - 1], dtype=np.uint64)
    for max_len in (1, 1000, 1023):
        got = fn(np.zeros(max_len + 1, dtype=np.uint64), lens)
        assert got.tobytes() == lens.astype(np.float64).tobytes()


def eff_check_one_bin(fn, Err):
    for l in (1, 250, 1000):
        c = np.zeros(1001, dtype=np.uint64); c[l] = 12345
        lens = np.array(sorted({1, max(1, l - 1), l, l + 1, 1000, 1001, 54321, 2 ** 32 - 1}), dtype=np.uint64)
        got = fn(c, lens)
        exp = np.array([float(L + 1 - l) if L >= l else float(L) for L in (int(x) for x in lens)])
        assert got.tobytes() == exp.tobytes(), (l, got, exp)


def eff_check_random(fn, Err):
    rng = np.random.default_rng(43)
    c = rng.integers(0, 1 << 20, 1001).astype(np.uint64); c[0] = 0; c[1:40] = 0
    lens = rng.integers(1, 200000, 10000).astype(np.uint64); lens[:1000] = rng.integers(1, 1100, 1000)
    got = fn(c, lens)
    assert np.isfinite(got).all() and (got >= 1.0).all()
    assert got.tobytes() == eff_lens(c, lens).tobytes()


def eff_check_errors(fn, Err):
    import pytest
    c = np.zeros(1001, dtype=np.uint64); c[0] = 1; c[200] = 5
    with pytest.raises(Err, match="-1"):                             # QM_E_ARG: bin 0 is never used
        fn(c, np.array([500], dtype=np.uint64))
    c[0] = 0
    with pytest.raises(Err, match="-1"):                             # QM_E_ARG: a transcript of length 0
        fn(c, np.array([500, 0], dtype=np.uint64))
    big = np.zeros(1001, dtype=np.uint64); big[1000] = 2 ** 53 // 1000 + 1   # Q reaches 2^53
    with pytest.raises(Err, match="-4"):                             # QM_E_UNSUPPORTED
        fn(big, np.array([500], dtype=np.uint64))
    big[1000] = 2 ** 53 // 1000; big[1] = 2 ** 53 - 1000 * (2 ** 53 // 1000)   # Q == 2^53 exactly
    with pytest.raises(Err, match="-4"):
        fn(big, np.array([500], dtype=np.uint64))
    big[1] -= 1                                                      # Q == 2^53 - 1: the largest that is taken
    assert fn(big, np.array([2000], dtype=np.uint64)).tobytes() == eff_lens(big, [2000]).tobytes()
    huge = np.zeros(1001, dtype=np.uint64); huge[1000] = 2 ** 63     # l * count wraps 64 bits
    with pytest.raises(Err, match="-4"):
        fn(huge, np.array([500], dtype=np.uint64))
    with pytest.raises(Err, match="-4"):                             # max_len 1024
        fn(np.zeros(1025, dtype=np.uint64), np.array([500], dtype=np.uint64))


EFF_CHECKS = {f.__name__[10:]: f for f in (eff_check_lengths, eff_check_empty, eff_check_one_bin, eff_check_random, eff_check_errors)}
