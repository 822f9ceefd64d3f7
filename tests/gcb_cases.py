"""Inputs, the restatements and the checks of the fragment GC bias tests (test_gc_bias.py: lane emulation and the host arithmetic,
test_gc_bias_gpu.py: device).  Everything here is exact: integer counts, and floats compared bit for bit.

A WORLD is a text with its transcripts: {"text": uint8[n], "off": int64[T], "lens": int64[T]}.  window_gc / classify / expect restate
the model of include/qmap_mi355.h in numpy over a prefix sum of the GC characters; eff_lens restates the closing arithmetic in
float64, every operation on its own and every float sum an explicit ascending loop.  A check takes the world and
`new(max_len, max_blocks)`, which makes an object over that world with add_hits / add_counts / counts / stat / expect / window_gc /
clear / close -- rapmap_amd.GCBias on the device, emu_gcb.EmuGcb under the lane emulation."""
import numpy as np

from rapmap_amd.api import HIT_DTYPE

NB = 25
CATS = ("used", "unmapped", "multi", "not_paired", "same_strand", "out_of_range", "overhang")
STATS = ("units",) + CATS
U, UNM, MULTI, NP, SS, OOR, OVH = range(7)


# ---- worlds

def make_world(seqs):
    """transcripts (bytes) laid out as an index lays them out: each followed by a `$`"""
    text = bytearray(); off = []
    for s in seqs:
        off.append(len(text)); text += s + b"$"
    return {"text": np.frombuffer(bytes(text), dtype=np.uint8).copy(), "off": np.asarray(off, dtype=np.int64), "lens": np.asarray([len(s) for s in seqs], dtype=np.int64)}


def _rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)])


PLAIN_LENS = (1, 2, 63, 64, 65, 127, 128, 129, 1000)                 # transcript starts at every kind of alignment within a 64-character block


def crafted_seqs(plain_only=False):
    """the transcripts of the crafted world; plain_only: upper-case ACGT only (what an index built from a FASTA file keeps)"""
    rng = np.random.default_rng(2024)
    seqs = [_rand_seq(rng, n) for n in PLAIN_LENS]
    seqs += [b"GC" * 50 + b"G", b"AT" * 50 + b"A", b"GA" * 65, _rand_seq(rng, 5000), b"C", b"T", _rand_seq(rng, 64, b"GC"), _rand_seq(rng, 200, b"AAAGCT")]
    if not plain_only:
        seqs += [_rand_seq(rng, 90, b"acgt"), _rand_seq(rng, 70, b"ACGTN"), _rand_seq(rng, 130, b"ACGTacgtNn"), b"gcGC" * 20]
    return seqs


def is_gc(text):
    t = np.asarray(text, dtype=np.uint8)
    return (t == ord("G")) | (t == ord("C")) | (t == ord("g")) | (t == ord("c"))


def gc_cum(world):
    c = np.zeros(world["text"].size + 1, dtype=np.int64)
    np.cumsum(is_gc(world["text"]), out=c[1:])
    return c


# ---- restatements

def window_gc(world, tids, starts, lens):
    """int32: GC characters of [start, start + len) of the transcript; -1 where the window is empty or does not lie on it"""
    cum = gc_cum(world); T = world["lens"].size
    out = np.full(len(tids), -1, dtype=np.int32)
    for i, (t, s, l) in enumerate(zip(tids, starts, lens)):
        t, s, l = int(t), int(s), int(l)
        if t < T and s >= 0 and l >= 1 and s + l <= int(world["lens"][t]):
            o = int(world["off"][t])
            out[i] = cum[o + s + l] - cum[o + s]
    return out


def bin_of(g, n):
    return np.minimum(NB - 1, (np.asarray(g, dtype=np.int64) * NB) // np.asarray(n, dtype=np.int64))


def classify(world, hit_offsets, hits, max_len):
    """-> (obs uint64[25], stats): every unit in the first category whose condition holds"""
    off = np.asarray(hit_offsets, dtype=np.int64)
    n = len(off) - 1
    cnt = np.diff(off)
    st = dict.fromkeys(STATS, 0)
    st["units"] = n
    st["unmapped"] = int(np.count_nonzero(cnt == 0)); st["multi"] = int(np.count_nonzero(cnt >= 2))
    obs = np.zeros(NB, dtype=np.uint64)
    one = off[:-1][cnt == 1]
    if one.size:
        h = np.asarray(hits)[one]
        fl = h["frag_len"].astype(np.int64)                         # unsigned 32-bit numbers
        not_paired = h["mate_status"] != 3
        same = ~not_paired & (h["fwd"] == h["mate_is_fwd"])
        oor = ~not_paired & ~same & ((fl == 0) | (fl > max_len))
        rest = ~not_paired & ~same & ~oor
        T = world["lens"].size
        tid = h["tid"].astype(np.int64)
        s = np.minimum(np.maximum(h["pos"].astype(np.int64), 0), np.maximum(h["mate_pos"].astype(np.int64), 0))
        e = s + fl
        known = tid < T
        L = np.where(known, world["lens"][np.where(known, tid, 0)], -1)
        ovh = rest & (~known | (e > L))
        used = rest & ~ovh
        st["not_paired"] = int(not_paired.sum()); st["same_strand"] = int(same.sum()); st["out_of_range"] = int(oor.sum())
        st["overhang"] = int(ovh.sum()); st["used"] = int(used.sum())
        if used.any():
            cum = gc_cum(world)
            o = world["off"][tid[used]]
            g = cum[o + e[used]] - cum[o + s[used]]
            obs += np.bincount(bin_of(g, fl[used]), minlength=NB).astype(np.uint64)
    assert sum(st[k] for k in CATS) == n and int(obs.sum()) == st["used"]
    return obs, st


def prefix_sums(counts):
    c = [int(x) for x in counts]
    P = [0] * len(c); Q = [0] * len(c)
    for l in range(1, len(c)):
        P[l] = P[l - 1] + c[l]; Q[l] = Q[l - 1] + l * c[l]
    return P, Q


def expect(world, counts):
    """H uint64[T][25]: per transcript and length, the bins of all windows from two slices of the prefix sum"""
    cum = gc_cum(world); c = [int(x) for x in counts]; max_len = len(c) - 1
    T = world["lens"].size
    H = np.zeros((T, NB), dtype=np.uint64)
    for t in range(T):
        L, o = int(world["lens"][t]), int(world["off"][t])
        row = [0] * NB
        for l in range(1, min(L, max_len) + 1):
            if c[l]:
                g = cum[o + l: o + L + 1] - cum[o: o + L - l + 1]
                for b, k in enumerate(np.bincount(bin_of(g, l), minlength=NB)):
                    row[b] += c[l] * int(k)
        H[t] = np.array(row, dtype=np.uint64)
    return H


def assert_identity(world, counts, H, what=""):
    """sum over b of H[t][b] == (L + 1) * P[m] - Q[m], m = min(L, max_len)"""
    P, Q = prefix_sums(counts)
    for t, L in enumerate(int(x) for x in world["lens"]):
        m = min(L, len(P) - 1)
        assert sum(int(x) for x in H[t]) == (L + 1) * P[m] - Q[m], (what, t, L)


def eff_lens(counts, lens, H, alpha, obs):
    """(eff, exp, ratio) in float64: one operation per line, float sums in explicit ascending loops"""
    P, _ = prefix_sums(counts); max_len = len(P) - 1
    H = np.asarray(H, dtype=np.uint64).reshape(-1, NB); T = H.shape[0]
    S = [sum(int(x) for x in H[t]) for t in range(T)]
    Hd = H.astype(np.float64)                                       # (double)H[t][b]
    ex = np.zeros(NB, dtype=np.float64)
    for t in range(T):                                               # ascending t; the 25 bins side by side
        if alpha[t] > 0 and S[t] > 0:
            share = Hd[t] / np.float64(S[t])
            w = np.float64(alpha[t]) * share
            ex = ex + w
    O = sum(int(x) for x in obs)
    E = np.float64(0.0)
    for b in range(NB):
        E = E + ex[b]
    ratio = np.ones(NB, dtype=np.float64)
    for b in range(NB):
        if O == 0 or E == 0.0 or ex[b] == 0.0:
            continue
        po = np.float64(int(obs[b])) / np.float64(O)
        pe = ex[b] / E
        r = po / pe
        ratio[b] = min(max(r, np.float64(1e-3)), np.float64(1e3))
    M = np.array([P[min(int(L), max_len)] for L in lens], dtype=np.uint64)
    s = np.zeros(T, dtype=np.float64)
    for b in range(NB):                                              # ascending b; the transcripts side by side
        w = ratio[b] * Hd[:, b]
        s = s + w
    eff = np.asarray(lens, dtype=np.uint64).astype(np.float64)
    nz = M > 0
    eff[nz] = s[nz] / M[nz].astype(np.float64)
    return eff, ex, ratio


# ---- observed sweep: case builders

def build(world, cats, max_len, rng, multi_sizes=(2, 3)):
    """units of the given categories -> (hit_offsets, hits).  Every record of a unit with hits would be `used` if it stood alone and
    unchanged, except for the one field the unit's category turns in its first record"""
    cats = np.asarray(cats, dtype=np.int64)
    n = cats.size; T = world["lens"].size
    k = np.ones(n, dtype=np.int64)
    k[cats == UNM] = 0
    nm = int(np.count_nonzero(cats == MULTI))
    if nm:
        k[cats == MULTI] = rng.choice(np.asarray(multi_sizes), size=nm)
    off = np.zeros(n + 1, dtype=np.int64); np.cumsum(k, out=off[1:])
    nh = int(off[-1])
    h = np.zeros(nh, dtype=HIT_DTYPE)
    h["read_len"] = rng.integers(0, 300, nh); h["mate_len"] = rng.integers(0, 300, nh)
    h["is_paired"] = rng.integers(0, 2, nh); h["aln_score"] = rng.integers(-100, 100, nh)
    h["mate_status"] = 3
    h["fwd"] = rng.integers(0, 2, nh); h["mate_is_fwd"] = 1 - h["fwd"]
    tid = rng.integers(0, T, nh); L = world["lens"][tid]
    f = rng.integers(1, np.minimum(L, max_len) + 1)                  # 1 .. min(L, max_len)
    s = rng.integers(0, L - f + 1)                                   # the window lies on the transcript: s + f <= L
    edge = rng.integers(0, 4, nh)
    s = np.where(edge == 0, L - f, s)                                # a quarter end exactly at L
    a = s.copy(); b = s + rng.integers(0, 60, nh)
    neg = (s == 0) & (rng.integers(0, 2, nh) == 1)
    a = np.where(neg, -rng.integers(1, 30, nh), a)                   # a negative position counts as 0
    swap = rng.integers(0, 2, nh) == 1
    h["tid"] = tid; h["frag_len"] = f
    h["pos"] = np.where(swap, b, a); h["mate_pos"] = np.where(swap, a, b)
    first = off[:-1]
    i = first[cats == NP]
    h["mate_status"][i] = rng.integers(0, 3, i.size)
    i = first[cats == SS]
    h["mate_is_fwd"][i] = h["fwd"][i]
    i = first[cats == OOR]
    h["frag_len"][i] = rng.choice(np.array([0, max_len + 1, 0x7fffffff, 0xffffffff, max_len + 7], dtype=np.uint32), size=i.size)
    i = first[cats == OVH]
    kind = rng.integers(0, 3, i.size)
    # the three ways to hang over: the window ends one character past the end; it starts far away; there is no such transcript
    Li = world["lens"][h["tid"][i]].astype(np.int64); fi = h["frag_len"][i].astype(np.int64)
    past = Li + 1 - fi                                               # >= 1: f <= L
    far = Li + rng.integers(0, 1 << 20, i.size)
    p = np.where(kind == 0, past, np.where(kind == 1, far, h["pos"][i]))
    m = np.where(kind == 0, past + rng.integers(0, 9, i.size), np.where(kind == 1, far + 5, h["mate_pos"][i]))
    h["pos"][i] = p; h["mate_pos"][i] = m
    beyond = np.where(rng.integers(0, 2, i.size) == 1, np.uint64(T), rng.integers(T, 1 << 32, i.size, dtype=np.uint64))
    h["tid"][i] = np.where(kind == 2, beyond, h["tid"][i].astype(np.uint64)).astype(np.uint32)
    return off, h


def random_batch(world, n, max_len, seed, every_wave=True):
    """n units of random categories; with every_wave the first seven units of every 64 hold the seven categories"""
    rng = np.random.default_rng(seed)
    cats = rng.integers(0, 7, n)
    if every_wave:
        for b in range(0, n - 6, 64):
            cats[b:b + 7] = rng.permutation(7)
    return build(world, cats, max_len, rng)


def fold_once(new, off, hits, max_len=1000, max_blocks=0):
    f = new(max_len, max_blocks)
    try:
        f.add_hits(off, hits)
        return f.counts(), f.stat()
    finally:
        f.close()


def assert_same(got_obs, got_stat, obs, st, what):
    assert np.array_equal(np.asarray(got_obs, dtype=np.uint64), obs), "%s: bins differ: %r, expected %r" % (what, got_obs, obs)
    assert {k: int(got_stat[k]) for k in STATS} == st, "%s: counters differ: %r, expected %r" % (what, {k: int(got_stat[k]) for k in STATS}, st)
    assert sum(int(got_stat[k]) for k in CATS) == int(got_stat["units"]), what


def check_against_restatement(world, new, off, hits, max_len=1000, max_blocks=0, what=""):
    c, s = fold_once(new, off, hits, max_len, max_blocks)
    eo, es = classify(world, off, hits, max_len)
    assert_same(c, s, eo, es, what)
    return eo, es


# ---- the checks of the rank structure and window_gc

def check_window_gc(world, new):
    g = new(1000, 0)
    try:
        q = []
        for t, L in enumerate(int(x) for x in world["lens"]):
            o = int(world["off"][t])
            q += [(t, 0, L), (t, 0, 1), (t, L - 1, 1), (t, 0, L + 1), (t, L, 1), (t, -1, 1), (t, 0, 0), (t, 1, L)]   # whole, ends, one past, empty
            # windows that start or end on a block boundary of the text, and one either side
            for p in range(((o + 63) // 64) * 64, o + L + 1, 64):
                for d in (-1, 0, 1):
                    s = p + d - o
                    if 0 <= s < L:
                        q += [(t, s, 1), (t, s, L - s), (t, 0, s if s else 1), (t, s, min(64, L - s)), (t, s, min(65, L - s))]
        T = world["lens"].size
        q += [(T, 0, 1), (0xffffffff, 0, 1)]
        rng = np.random.default_rng(5)
        for _ in range(3000):
            t = int(rng.integers(0, T)); L = int(world["lens"][t]); s = int(rng.integers(0, L)); q.append((t, s, int(rng.integers(1, L - s + 1))))
        tids, starts, lens = (np.array(x) for x in zip(*q))
        got = g.window_gc(tids.astype(np.uint32), starts, lens)
        exp = window_gc(world, tids, starts, lens)
        assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:10]
        assert (exp == -1).sum() >= 4 * T and (exp == lens).any() and ((exp == 0) & (lens > 50)).any()   # refusals, all-GC and all-AT windows are there
        assert g.window_gc([], [], []).size == 0
    finally:
        g.close()


# ---- the checks of the expected matrix

def histograms(world, max_len):
    """name -> counts uint64[max_len + 1]"""
    rng = np.random.default_rng(9)
    z = lambda: np.zeros(max_len + 1, dtype=np.uint64)
    out = {"empty": z()}
    c = z(); c[min(200, max_len)] = 7; out["a single length"] = c
    for L in sorted({int(x) for x in world["lens"]}):
        if L + 1 <= max_len:
            c = z(); c[1] = 3; c[L] = 5; c[L + 1] = 11; c[max_len] = 2; out["1, L, L + 1, max_len at L = %d" % L] = c
    c = z(); c[1: min(300, max_len) + 1] = rng.integers(1, 1000, min(300, max_len)).astype(np.uint64); out["every length 1..300"] = c
    c = z(); c[rng.integers(1, max_len + 1, 12)] = rng.integers(1, 1 << 20, 12).astype(np.uint64); out["sparse"] = c
    c = z(); c[rng.integers(1, max_len + 1, 20)] = (np.uint64(1 << 32) - rng.integers(0, 3, 20).astype(np.uint64)); c[1] = (1 << 32) + 1; out["counts near 2^32"] = c
    return out


def _check_expect(world, new, max_len, max_blocks, names=None):
    g = new(max_len, max_blocks)
    out = {}
    try:
        T = world["lens"].size
        for name, c in histograms(world, max_len).items():
            if names is not None and name not in names:
                continue
            H = g.expect(c, T)
            exp = expect(world, c)
            assert H.dtype == np.uint64 and H.shape == (T, NB)
            assert np.array_equal(H, exp), "%s, max_len %d, max_blocks %d: rows %r differ" % (name, max_len, max_blocks, np.flatnonzero((H != exp).any(axis=1))[:10])
            assert_identity(world, c, H, name)
            out[name] = H
        return out
    finally:
        g.close()


def check_expect_default_grid(world, new):
    got = _check_expect(world, new, 1000, 0)
    assert not got["empty"].any() and got["every length 1..300"].any(axis=1).all()
    assert len(got) >= 8


def check_expect_max_len_1(world, new):
    _check_expect(world, new, 1, 0)


def check_expect_max_len_1023(world, new):
    _check_expect(world, new, 1023, 0, names=("every length 1..300", "sparse", "counts near 2^32", "1, L, L + 1, max_len at L = 1000", "1, L, L + 1, max_len at L = 64"))


def check_expect_grid_caps(world, new):
    """one and two workgroups against the default grid: the same bits"""
    names = ("every length 1..300", "counts near 2^32")
    a = _check_expect(world, new, 1000, 0, names); b = _check_expect(world, new, 1000, 1, names); c = _check_expect(world, new, 1000, 2, names)
    for k in names:
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes()


def check_expect_twice_and_clear(world, new):
    g = new(1000, 0)
    try:
        T = world["lens"].size
        hs = histograms(world, 1000)
        a = g.expect(hs["sparse"], T)
        off, h = random_batch(world, 300, 1000, seed=4)
        g.add_hits(off, h)
        g.clear()
        b = g.expect(hs["sparse"], T); c = g.expect(hs["every length 1..300"], T); d = g.expect(hs["sparse"], T)
        assert a.tobytes() == b.tobytes() == d.tobytes() and np.array_equal(c, expect(world, hs["every length 1..300"]))   # nothing is left over from call to call
        assert not g.counts().any()
    finally:
        g.close()


def check_expect_refusals(world, new, Err=Exception):
    g = new(1000, 0)
    try:
        T = world["lens"].size; Lmax = int(world["lens"].max())
        c = np.zeros(1001, dtype=np.uint64)
        c[500] = (2 ** 63 + Lmax - 1) // Lmax                       # P * Lmax >= 2^63
        for bad, code in ((c, "-4"),):
            try:
                g.expect(bad, T)
            except Exception as e:
                assert code in str(e), e
            else:
                raise AssertionError("P * max L >= 2^63 was accepted")
        c[500] -= 1                                                  # the largest that is taken: P * Lmax < 2^63
        assert (c[500] * np.uint64(1)).item() * Lmax < 2 ** 63
        H = g.expect(c, T)
        assert_identity(world, c, H, "just below the refusal")
        c0 = np.zeros(1001, dtype=np.uint64); c0[0] = 1
        for bad, n in ((c0, T), (np.zeros(1001, dtype=np.uint64), T + 1)):
            try:
                g.expect(bad, n)
            except Exception as e:
                assert "-1" in str(e), e
            else:
                raise AssertionError("a bad argument was accepted")
    finally:
        g.close()


EXPECT_CHECKS = {f.__name__[6:]: f for f in (check_expect_default_grid, check_expect_max_len_1, check_expect_max_len_1023, check_expect_grid_caps,
                                             check_expect_twice_and_clear, check_expect_refusals)}


# ---- the checks of the observed sweep

SIZES = (0, 1, 63, 64, 65, 255, 257, 5000)


def check_sizes(world, new):
    for n in SIZES:
        off, h = random_batch(world, n, 1000, seed=100 + n)
        eo, es = check_against_restatement(world, new, off, h, what="%d units" % n)
        if n == 5000:                                                # every category present in every wavefront
            for b in range(0, n - 63, 64):
                _, sb = classify(world, off[b:b + 65] - off[b], h[off[b]:off[b + 64]], 1000)
                assert all(sb[k] > 0 for k in CATS), (b, sb)
            assert es["used"] > 500 and np.count_nonzero(eo) >= 10


def check_grid_caps(world, new):
    off, h = random_batch(world, 20001, 1000, seed=7)
    for mb in (1, 2, 0):
        check_against_restatement(world, new, off, h, max_blocks=mb, what="20 001 units, max_blocks %d" % mb)


def _one(world, tid, pos, mate_pos, frag_len):
    h = np.zeros(1, dtype=HIT_DTYPE)
    h["tid"] = tid; h["pos"] = pos; h["mate_pos"] = mate_pos; h["frag_len"] = frag_len; h["mate_status"] = 3; h["fwd"] = 1; h["mate_is_fwd"] = 0
    return h


def check_edges(world, new):
    """by hand: windows ending at L and L + 1, negative positions, tid == n_txps, g == n and g == 0, the fragment-length edges"""
    lens = [int(x) for x in world["lens"]]; T = len(lens)
    cum = gc_cum(world)
    gcs = [int(cum[int(o) + L] - cum[int(o)]) for o, L in zip(world["off"], lens)]
    t_gc = next(t for t in range(T) if gcs[t] == lens[t] and lens[t] >= 50)     # all G / C
    t_at = next(t for t in range(T) if gcs[t] == 0 and lens[t] >= 50)           # no G / C
    t_k = lens.index(1000)
    for max_len in (1000, 40):
        rows = [  # (record, category, bin or None)
            (_one(world, t_gc, 10, 3, 30), "used", NB - 1), (_one(world, t_at, 3, 10, 30), "used", 0),
            (_one(world, t_gc, lens[t_gc] - 30, lens[t_gc] - 5, 30), "used", NB - 1),          # ends exactly at L
            (_one(world, t_gc, lens[t_gc] - 29, lens[t_gc] - 5, 30), "overhang", None),        # ... at L + 1
            (_one(world, t_gc, -7, 20, 30), "used", NB - 1), (_one(world, t_at, 20, -7, 30), "used", 0), (_one(world, t_at, -1, -1, 30), "used", 0),
            (_one(world, T, 0, 0, 30), "overhang", None), (_one(world, 0xffffffff, 0, 0, 30), "overhang", None),
            (_one(world, t_k, 5, 9, 1), "used", None), (_one(world, t_k, 0, 0, max_len), "used", None), (_one(world, t_k, 1000 - max_len, 1000, max_len), "used", None),
            (_one(world, t_k, 0, 0, max_len + 1), "out_of_range", None), (_one(world, t_k, 0, 0, 0xffffffff), "out_of_range", None),
            (_one(world, t_k, 0, 0, 0), "out_of_range", None), (_one(world, T, 0, 0, 0), "out_of_range", None),
            (_one(world, lens.index(1), 0, 0, 1), "used", None), (_one(world, lens.index(1), 0, 1, 1), "used", None), (_one(world, lens.index(1), 1, 1, 1), "overhang", None),
            (_one(world, lens.index(2), 1, 1, 2), "overhang", None), (_one(world, lens.index(2), 0, 5, 2), "used", None),
        ]
        h = np.concatenate([r[0] for r in rows]); off = np.arange(len(rows) + 1, dtype=np.int64)
        for i, (rec, cat, b) in enumerate(rows):
            o1, s1 = classify(world, [0, 1], rec, max_len)
            assert s1[cat] == 1 and (b is None or o1[b] == 1), (i, cat, s1)     # the restatement agrees with the hand
        check_against_restatement(world, new, off, h, max_len=max_len, what="edges, max_len %d" % max_len)


def check_multi_units(world, new):
    rng = np.random.default_rng(11)
    cats = np.array([MULTI, U, MULTI, MULTI, UNM, MULTI, U] * 3)
    for sizes in ((2,), (3,), (200,), (2, 3, 200)):
        off, h = build(world, cats, 1000, rng, multi_sizes=sizes)
        first = off[:-1][np.diff(off) >= 2]
        _, alone = classify(world, np.arange(first.size + 1), h[first], 1000)
        assert alone["used"] == first.size                           # every first record would qualify if it were alone
        eo, es = check_against_restatement(world, new, off, h, what="units of %r hits" % (sizes,))
        assert es["multi"] == 12 and es["used"] == 6


def check_no_hits(world, new):
    for n in (1, 64, 300):
        off = np.zeros(n + 1, dtype=np.int64)
        for hits in (None, np.zeros(0, dtype=HIT_DTYPE)):
            c, s = fold_once(new, off, hits)
            assert not c.any() and s["unmapped"] == n == s["units"] and s["used"] == 0


def check_max_lens(world, new):
    for max_len in (1, 2, 1000, 1023):
        off, h = random_batch(world, 700, max_len, seed=max_len)
        h["frag_len"][::5] = max_len + 1                             # just beyond, whatever the unit's category
        eo, es = check_against_restatement(world, new, off, h, max_len=max_len, what="max_len %d" % max_len)
        assert es["used"] > 50 and es["out_of_range"] > 20


def check_accumulate_and_clear(world, new):
    a = random_batch(world, 3000, 1000, seed=21); b = random_batch(world, 777, 1000, seed=22)
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
    a = random_batch(world, 3000, 1000, seed=31); b = random_batch(world, 2049, 1000, seed=32)
    both = new(1000, 0); one = new(1000, 0); other = new(1000, 0)
    try:
        both.add_hits(*a); both.add_hits(*b)
        one.add_hits(*a); other.add_hits(*b)
        one.add_counts(other.counts())
        assert np.array_equal(one.counts(), both.counts())
        sb_, so = both.stat(), one.stat()
        # the counts bring their fragments only: `used` and the units grow by their sum, the other categories stay where they were swept
        _, sa = classify(world, *a, 1000); _, sbb = classify(world, *b, 1000)
        assert so["used"] == sb_["used"] == sa["used"] + sbb["used"]
        assert so["units"] == sa["units"] + sbb["used"] and sum(so[k] for k in CATS) == so["units"]
        for k in CATS[1:]:
            assert so[k] == sa[k] and sb_[k] == sa[k] + sbb[k]
    finally:
        both.close(); one.close(); other.close()


OBS_CHECKS = {f.__name__[6:]: f for f in (check_sizes, check_grid_caps, check_edges, check_multi_units, check_no_hits, check_max_lens,
                                          check_accumulate_and_clear, check_add_counts)}


# ---- the host arithmetic; `fn(counts, lens, H, alpha, obs)` is the implementation under test

def eff_inputs(T, seed, max_len=1000):
    """a histogram, T transcripts, a matrix with the identity's row sums (bins spread at random), estimates with zeros among them"""
    rng = np.random.default_rng(seed)
    c = np.zeros(max_len + 1, dtype=np.uint64); c[150:450] = rng.integers(0, 5000, 300).astype(np.uint64)
    P, Q = prefix_sums(c)
    lens = rng.integers(1, 20000, T).astype(np.uint64); lens[: T // 10] = rng.integers(1, 400, T // 10)
    H = np.zeros((T, NB), dtype=np.uint64)
    for t, L in enumerate(int(x) for x in lens):
        m = min(L, max_len); S = (L + 1) * P[m] - Q[m]
        w = rng.random(NB) ** 3; w[rng.integers(0, NB, 5)] = 0
        if w.sum() == 0:
            w[12] = 1
        row = np.floor(w / w.sum() * S).astype(np.uint64); row[int(np.argmax(w))] += np.uint64(S - int(row.sum()))
        H[t] = row
    alpha = rng.random(T) * 100; alpha[rng.integers(0, T, T // 7)] = 0.0
    obs = rng.integers(0, 100000, NB).astype(np.uint64)
    return c, lens, H, alpha, obs


def _same(fn, args, what):
    got = fn(*args); exp = eff_lens(*args)
    for g, e, name in zip(got, exp, ("eff", "exp", "ratio")):
        assert g.dtype == np.float64 and g.tobytes() == e.tobytes(), (what, name, g[:5], e[:5])
    return got


def eff_check_random(fn):
    args = eff_inputs(10000, 61)
    eff, ex, ratio = _same(fn, args, "10^4 transcripts")
    assert np.isfinite(eff).all() and (eff > 0).all() and (ratio != 1.0).any()


def eff_check_ratio_one(fn):
    c, lens, H, alpha, obs = eff_inputs(200, 62)
    P, _ = prefix_sums(c)
    plain = np.array([float(L) if P[min(int(L), 1000)] == 0 else float(sum(int(x) for x in H[t])) / float(P[min(int(L), 1000)]) for t, L in enumerate(lens)])
    # O == 0; E == 0 (alpha 0 everywhere); then single bins: an empty expected bin keeps ratio 1 whatever was observed there
    for a, o, what in ((alpha, np.zeros(NB, dtype=np.uint64), "O == 0"), (np.zeros(200), obs, "alpha == 0 everywhere")):
        eff, ex, ratio = _same(fn, (c, lens, H, a, o), what)
        assert (ratio == 1.0).all()
        # S_t / M_t up to the rounding of the 25-term sum
        assert np.allclose(eff, plain, rtol=1e-12, atol=0)
    H2 = H.copy(); H2[:, 3] = 0
    eff, ex, ratio = _same(fn, (c, lens, H2, alpha, obs), "an empty expected bin")
    assert ex[3] == 0.0 and ratio[3] == 1.0 and obs[3] > 0 and (ratio != 1.0).any()


def eff_check_clamps(fn):
    c, lens, H, alpha, obs = eff_inputs(200, 63)
    obs = obs.copy(); obs[:] = 1000; obs[5] = 0; obs[7] = 10 ** 12
    H = H.copy(); H[:, 7] = (H.sum(axis=1) > 0).astype(np.uint64)    # a bin that is next to never expected and often observed
    eff, ex, ratio = _same(fn, (c, lens, H, alpha, obs), "clamps")
    assert ratio[5] == 1e-3 and ratio[7] == 1e3 and ratio.min() == 1e-3 and ratio.max() == 1e3


def eff_check_no_fragment_fits(fn):
    c, lens, H, alpha, obs = eff_inputs(50, 64)
    lens = lens.copy(); lens[:10] = np.arange(1, 11); H = H.copy(); H[:10] = 0    # shorter than every fragment: M_t == 0
    eff, ex, ratio = _same(fn, (c, lens, H, alpha, obs), "M_t == 0")
    assert np.array_equal(eff[:10], np.arange(1, 11).astype(np.float64))


def eff_check_agrees_with_fld(fn, fld_fn):
    """with obs the rounded exp, every ratio is within rounding of 1 and e' of qm_fld's effective length: 1e-9 relative"""
    c, lens, H, alpha, obs = eff_inputs(2000, 65)
    alpha = alpha * 1e9                                              # exp of the order of 10^11 per bin: rounding it moves a ratio by 1e-11
    _, ex, _ = eff_lens(c, lens, H, alpha, np.zeros(NB, dtype=np.uint64))
    obs = np.rint(ex).astype(np.uint64)
    assert (obs[ex > 0] > 10 ** 10).all()
    eff, _, ratio = _same(fn, (c, lens, H, alpha, obs), "obs = rounded exp")
    ref = fld_fn(c, lens)
    assert np.abs(ratio - 1.0).max() < 1e-9
    assert (np.abs(eff - ref) <= 1e-9 * np.abs(ref)).all(), np.abs(eff / ref - 1).max()


EFF_CHECKS = {f.__name__[10:]: f for f in (eff_check_random, eff_check_ratio_one, eff_check_clamps, eff_check_no_fragment_fits)}


# ---- the planted bias: fragments thinned by the GC bin of their window

PLANTED_SEED = 77
PLANTED_DRAWS = 16000


def planted_keep():
    """the probability to keep a fragment, falling with its GC bin: 1.0 in bin 0 down to 0.1 in bin 24"""
    return 1.0 - 0.9 * np.arange(NB) / (NB - 1)


def _gc_seq(rng, n, p):
    """n characters, each G or C with probability p"""
    gc_ = rng.random(n) < p
    return np.where(gc_, np.frombuffer(b"GC", dtype=np.uint8)[rng.integers(0, 2, n)], np.frombuffer(b"AT", dtype=np.uint8)[rng.integers(0, 2, n)])


def planted_transcripts(seed=PLANTED_SEED):
    """-> (names, transcripts uint8, abundances).  40 transcripts of their own, each of three stretches of 500 characters, one GC-poor
    (25 .. 40 %), one in between (40 .. 60 %), one GC-rich (60 .. 75 %), in random order: they map uniquely, and since each holds windows
    of every bin, what is observed along ONE transcript shows the bias whatever that transcript's abundance (the model's expected counts
    are weighted by the first estimate, which has already taken up a bias that is the same all along a transcript).  10 genes of two
    isoforms: 450 shared characters at 50 % GC and 650 of the isoform's own, GC-rich (68 %) in one and GC-poor (32 %) in the other, the
    shared part in front in every other gene.  A fragment of the shared part maps to both isoforms: how the estimate splits those is what
    the effective lengths decide, so that is where a GC bias shows in NumReads."""
    rng = np.random.default_rng(seed)
    names, txps = [], []
    for i in range(40):
        p = np.array([rng.uniform(0.25, 0.4), rng.uniform(0.4, 0.6), rng.uniform(0.6, 0.75)])[rng.permutation(3)]
        names.append("S%d" % i); txps.append(np.concatenate([_gc_seq(rng, 500, x) for x in p]))
    for g in range(10):
        shared = _gc_seq(rng, 450, 0.5)
        for iso, p in (("A", 0.68), ("B", 0.32)):
            own = _gc_seq(rng, 650, p)
            names.append("G%d.%s" % (g, iso)); txps.append(np.concatenate([shared, own] if g % 2 == 0 else [own, shared]))
    theta = rng.uniform(0.5, 2.0, len(txps))
    return names, txps, theta


def planted_fragments(txps, theta, n_draws=PLANTED_DRAWS, seed=PLANTED_SEED + 1, read_len=60):
    """n_draws fragments: a transcript by abundance x length, a length of N(220, 20) clipped to [150, 300], a start uniform over the
    transcript; each kept with planted_keep() of its window's GC bin.  -> (reads1, reads2 as lists of bytes, mate 2 reverse-complemented,
    the mates swapped in half of the pairs; tid int64[kept] of the transcript each kept fragment came from)"""
    from rapmap_amd.synth import _COMP
    rng = np.random.default_rng(seed)
    lens = np.array([t.size for t in txps], dtype=np.int64)
    w = theta * lens
    tid = rng.choice(len(txps), size=n_draws, p=w / w.sum())
    flen = np.clip(rng.normal(220, 20, n_draws).astype(np.int64), 150, 300)
    start = (rng.random(n_draws) * (lens[tid] - flen + 1)).astype(np.int64)
    u = rng.random(n_draws); swap = rng.random(n_draws) < 0.5
    keep = planted_keep()
    r1, r2, origin = [], [], []
    for i in range(n_draws):
        f = txps[int(tid[i])][int(start[i]):int(start[i] + flen[i])]
        if u[i] >= keep[int(bin_of(int(is_gc(f).sum()), int(flen[i])))]:
            continue
        a = f[:read_len].tobytes(); b = _COMP[f[::-1][:read_len]].tobytes()
        if swap[i]:
            a, b = b, a
        r1.append(a); r2.append(b); origin.append(int(tid[i]))
    return r1, r2, np.array(origin, dtype=np.int64)
