"""Inputs, the restatements and the checks of the sequence-specific bias tests (test_seq_bias.py: lane emulation and the two host
functions, test_seq_bias_gpu.py: device).  Everything here is exact: integer counts, and floats compared bit for bit.

A WORLD is gcb_cases' ({"text", "off", "lens"}).  words / classify / expect / weights / ratios / eff_lens restate the model of
include/qmap_mi355.h in numpy and Python integers; eff_lens spells out the order of every float sum.  A check takes the world and
`new(max_len, max_blocks)`, which makes an object over that world with add_hits / add_counts / counts / stat / expect / eff_lens /
context / clear / close -- rapmap_amd.SeqBias on the device, emu_sqb.EmuSqb under the lane emulation."""
import math

import numpy as np

import gcb_cases as gc
from rapmap_amd.api import HIT_DTYPE

CTX, BINS, SHAPE = 9, 1152, (2, 9, 64)
CATS = ("used", "unmapped", "multi", "not_paired", "same_strand", "out_of_range", "overhang", "ambiguous")
STATS = ("units",) + CATS
LENS = (1, 2, 8, 9, 10, 13, 63, 64, 65, 127, 128, 129, 1000, 5000)   # shorter than a context, one context long, across every tile edge, beyond 64 + max_len

_CODE = np.full(256, 4, dtype=np.int64)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _i; _CODE[ord(_c.lower())] = _i


def crafted_seqs(plain_only=False):
    """the transcripts of the crafted world; plain_only: upper-case ACGT only (what an index built from a FASTA file keeps)"""
    rng = np.random.default_rng(2025)
    seqs = [gc._rand_seq(rng, n) for n in LENS]
    seqs += [b"CA" * 20, gc._rand_seq(rng, 300, b"AC"), gc._rand_seq(rng, 70)]
    if not plain_only:
        seqs += [gc._rand_seq(rng, 90, b"acgt"), gc._rand_seq(rng, 400, b"ACGTACGTACGTACGTACGTN"), gc._rand_seq(rng, 130, b"ACGTacgtACGTacgtNn"), b"ACGTN" + b"ACGTACGTA" + b"n",
                 b"ACGTACGTA" + b"N" + b"ACGTACGTA"]
    return seqs


def codes(world):
    return _CODE[np.asarray(world["text"], dtype=np.uint8)]


# ---- restatements

def _words_of(ch):
    """ch int64[n][9] characters c_0 .. c_8 -> words int64[n][9]"""
    w = np.empty_like(ch)
    w[:, 0] = ch[:, 0]; w[:, 1] = 4 * ch[:, 0] + ch[:, 1]
    for j in range(2, CTX):
        w[:, j] = 16 * ch[:, j - 2] + 4 * ch[:, j - 1] + ch[:, j]
    return w


def contexts(code, o, L, pos, end):
    """the contexts of `end` at the positions pos (int64[n]) of the transcript at text offset o, length L:
    (status int64[n]: 0 valid, 1 not on the transcript, 2 ambiguous; words int64[n][9], rows of -1 where not valid)"""
    pos = np.asarray(pos, dtype=np.int64)
    on = (pos >= 3) & (pos <= L - 6) if end == 0 else (pos >= 5) & (pos <= L - 4)
    status = np.where(on, 0, 1)
    words = np.full((pos.size, CTX), -1, dtype=np.int64)
    p = pos[on]
    if p.size:
        j = np.arange(CTX)
        idx = o + p[:, None] - 3 + j[None, :] if end == 0 else o + p[:, None] + 3 - j[None, :]
        ch = code[idx]
        amb = (ch > 3).any(axis=1)
        if end == 1:
            ch = 3 - ch
        w = _words_of(np.where(ch < 0, 0, ch))
        w[amb] = -1
        words[on] = w
        st = status[on]; st[amb] = 2; status[on] = st
    return status, words


def probe(world, tids, positions, ends):
    """int32[n][9]: what qm_sqb_context answers"""
    code = codes(world); T = world["lens"].size
    out = np.full((len(tids), CTX), -1, dtype=np.int32)
    for i, (t, p, e) in enumerate(zip(tids, positions, ends)):
        t, p, e = int(t), int(p), int(e)
        if t < T and e in (0, 1):
            out[i] = contexts(code, int(world["off"][t]), int(world["lens"][t]), [p], e)[1][0]
    return out


def classify(world, hit_offsets, hits, max_len):
    """-> (obs uint64[2][9][64], stats): every unit in the first category whose condition holds"""
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
        code = codes(world); T = world["lens"].size
        h = h[rest]; fl = fl[rest]
        tid = h["tid"].astype(np.int64)
        s = np.minimum(np.maximum(h["pos"].astype(np.int64), 0), np.maximum(h["mate_pos"].astype(np.int64), 0)); i = s + fl - 1
        known = tid < T
        L = np.where(known, world["lens"][np.where(known, tid, 0)], -1); o = np.where(known, world["off"][np.where(known, tid, 0)], 0)
        on = known & (i + 1 <= L) & (s >= 3) & (s <= L - 6) & (i >= 5) & (i <= L - 4)
        st["overhang"] = int((~on).sum())
        j = np.arange(CTX)
        c5 = code[(o[on] + s[on])[:, None] - 3 + j[None, :]]; c3 = code[(o[on] + i[on])[:, None] + 3 - j[None, :]]
        amb = (c5 > 3).any(axis=1) | (c3 > 3).any(axis=1)
        st["ambiguous"] = int(amb.sum()); st["used"] = int((~amb).sum())
        w5 = _words_of(c5[~amb]); w3 = _words_of(3 - c3[~amb])
        for jj in range(CTX):
            obs[0, jj] += np.bincount(w5[:, jj], minlength=64).astype(np.uint64); obs[1, jj] += np.bincount(w3[:, jj], minlength=64).astype(np.uint64)
    assert sum(st[k] for k in CATS) == n and int(obs.sum()) == 18 * st["used"]
    return obs, st


def prefix(counts):
    c = [int(x) for x in counts]
    P = [0] * len(c)
    for l in range(1, len(c)):
        P[l] = P[l - 1] + c[l]
    return P


_valid_cache = {}


def _valid_words(code, o, L, end):
    """(positions, words) of the valid contexts of one end of a transcript (kept: the restatements ask again and again)"""
    key = (code[o:o + L].tobytes(), end)
    if key not in _valid_cache:
        pos = np.arange(L, dtype=np.int64)
        st, w = contexts(code, o, L, pos, end)
        ok = st == 0
        _valid_cache[key] = (pos[ok], w[ok])
    return _valid_cache[key]


def expect(world, counts, q):
    """(exp uint64[2][9][64] in Python integers' arithmetic, the two totals sum_t q_t sum_valid P[.] per end)"""
    P = prefix(counts); m = len(P) - 1
    Pa = np.array(P, dtype=object)
    code = codes(world)
    ex = np.zeros(SHAPE, dtype=object); totals = [0, 0]
    for t, (o, L) in enumerate(zip((int(x) for x in world["off"]), (int(x) for x in world["lens"]))):
        qt = int(q[t])
        if not qt:
            continue
        for end in (0, 1):
            pos, w = _valid_words(code, o, L, end)
            if not pos.size:
                continue
            d = np.minimum(m, L - pos) if end == 0 else np.minimum(m, pos + 1)
            wt = Pa[d] * qt
            totals[end] += int(wt.sum())
            for j in range(CTX):
                np.add.at(ex[end, j], w[:, j], wt)
    assert all(int(ex[e, j].sum()) == totals[e] for e in (0, 1) for j in range(CTX))
    assert max(totals) < 2 ** 64
    return ex.astype(np.uint64), totals


def assert_nine_sums(ex, totals=None, what=""):
    """for each end, the sum over w of exp[end][j][w] is the same for all nine j (and the restated total)"""
    for e in (0, 1):
        sums = {sum(int(x) for x in ex[e, j]) for j in range(CTX)}
        assert len(sums) == 1, (what, e, sums)
        if totals is not None:
            assert sums == {totals[e]}, (what, e)


def ilogb(x):
    return math.frexp(x)[1] - 1


def weights(alpha, lens, counts):
    """(q uint64[T], k): one operation per line, the float sum an explicit ascending loop"""
    c = [int(x) for x in counts]; m = len(c) - 1
    P = prefix(c); Q = [0] * len(c)
    for l in range(1, len(c)):
        Q[l] = Q[l - 1] + l * c[l]
    T = len(lens)
    rho = [0.0] * T
    X = 0.0
    for t in range(T):
        L = int(lens[t]); mm = min(L, m)
        S = (L + 1) * P[mm] - Q[mm]
        if float(alpha[t]) > 0.0 and S:
            rho[t] = float(alpha[t]) / float(S)
        w = rho[t] * float(L)
        X = X + w
    z = X * float(P[m])
    if z == 0.0:
        return np.zeros(T, dtype=np.uint64), 0
    k = 61 - ilogb(z)
    return np.array([int(math.floor(math.ldexp(r, k))) for r in rho], dtype=np.uint64), k


def weight_bound(q, lens, counts):
    """sum of q_t * L_t * P[m] in Python integers"""
    return sum(int(a) * int(b) for a, b in zip(q, lens)) * prefix(counts)[-1]


def ratios(obs, ex):
    obs = np.asarray(obs, dtype=np.uint64).reshape(SHAPE); ex = np.asarray(ex, dtype=np.uint64).reshape(SHAPE)
    R = np.ones(SHAPE, dtype=np.float64)
    for e in (0, 1):
        for j in range(CTX):
            for w in range(4 if j == 0 else 16 if j == 1 else 64):
                g = w & ~3
                so = sum(int(x) for x in obs[e, j, g:g + 4]); se = sum(int(x) for x in ex[e, j, g:g + 4])
                po = np.float64(int(obs[e, j, w]) + 1) / np.float64(so + 4)
                pe = np.float64(int(ex[e, j, w]) + 1) / np.float64(se + 4)
                R[e, j, w] = min(max(po / pe, np.float64(0.25)), np.float64(4.0))
    return R


def bias(code, o, L, R, end):
    """b5 (end 0) or b3 (end 1) at every position of a transcript: ((1.0 * R[0]) * R[1]) ... over ascending j, 1.0 without a valid context"""
    pos, w = _valid_words(code, o, L, end)
    b = np.ones(L, dtype=np.float64)
    if pos.size:
        v = np.ones(pos.size, dtype=np.float64)
        for j in range(CTX):
            v = v * R[end, j, w[:, j]]
        b[pos] = v
    return b


def tile_sums(v):
    """the tree of wave_sum_f64 over every 64 consecutive values (absent ones 0.0) -> float64[tiles]"""
    n = (v.size + 63) // 64
    x = np.zeros(n * 64, dtype=np.float64); x[:v.size] = v
    x = x.reshape(n, 4, 16)
    s = x[:, :, 0::2] + x[:, :, 1::2]                                # (x0 + x1), (x2 + x3), ...
    s = s[:, :, 0::2] + s[:, :, 1::2]                                # the quads
    s = s[:, :, 0::2] + s[:, :, 1::2]                                # the halves of a row
    s = s[:, :, 0] + s[:, :, 1]                                      # the rows
    return (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])


def eff_lens(world, counts, R, any_order=False):
    """e' float64[T] in the header's order.  any_order: another order altogether -- the lengths descending, the starts of a length
    backwards through np.sum's pairwise tree; for inputs whose every partial sum is exact"""
    R = np.asarray(R, dtype=np.float64).reshape(SHAPE)
    c = [int(x) for x in counts]; m = len(c) - 1; P = prefix(c)
    code = codes(world)
    out = np.zeros(world["lens"].size, dtype=np.float64)
    for t, (o, L) in enumerate(zip((int(x) for x in world["off"]), (int(x) for x in world["lens"]))):
        M = P[min(L, m)]
        if not M:
            out[t] = float(L); continue
        b5 = bias(code, o, L, R, 0); b3 = bias(code, o, L, R, 1)
        if any_order:
            N = np.float64(0.0)
            for l in range(min(m, L), 0, -1):                        # descending lengths, whole rows at once
                if c[l]:
                    N = N + np.float64(c[l]) * np.sum((b5[:L - l + 1] * b3[l - 1:])[::-1])
            out[t] = N / np.float64(M); continue
        a = np.zeros(L, dtype=np.float64)
        for l in range(1, min(m, L) + 1):
            if c[l]:
                p = np.float64(c[l]) * b3[l - 1:]
                a[:L - l + 1] = a[:L - l + 1] + p
        v = b5 * a
        N = np.float64(0.0)
        for x in tile_sums(v):
            N = N + x
        out[t] = N / np.float64(M)
    return out


def fld_quotient(world, counts):
    """S_t / P[min(L_t, m)]: the fragment-length model's effective length as one quotient"""
    c = [int(x) for x in counts]; m = len(c) - 1; P = prefix(c); Q = [0] * len(c)
    for l in range(1, len(c)):
        Q[l] = Q[l - 1] + l * c[l]
    out = []
    for L in (int(x) for x in world["lens"]):
        mm = min(L, m)
        out.append(float(L) if not P[mm] else np.float64((L + 1) * P[mm] - Q[mm]) / np.float64(P[mm]))
    return np.array(out, dtype=np.float64)


# ---- the checks of the contexts

def check_contexts(world, new):
    g = new(1000, 0)
    try:
        q = []
        T = world["lens"].size
        for t, L in enumerate(int(x) for x in world["lens"]):
            if L <= 130:
                q += [(t, p, e) for p in range(-2, L + 3) for e in (0, 1)]
            else:
                q += [(t, p, e) for p in (0, 2, 3, 4, 5, 6, L - 7, L - 6, L - 5, L - 4, L - 3, L - 1, L) for e in (0, 1)]
        q += [(T, 5, 0), (0xffffffff, 5, 1), (T - 1, 5, 2), (T - 1, 5, -1), (T - 1, -2 ** 31, 0), (T - 1, 2 ** 31 - 1, 1)]
        tids, pos, ends = (np.array(x) for x in zip(*q))
        got = g.context(tids.astype(np.uint32), pos, ends)
        exp = probe(world, tids, pos, ends)
        assert got.shape == exp.shape and np.array_equal(got, exp), np.flatnonzero((got != exp).any(axis=1))[:10]
        valid = exp[:, 0] >= 0
        assert valid.sum() > 500 and (~valid).sum() > 200 and exp.max() == 63 and ((exp >= 0).all(axis=1) == valid).all()
        assert g.context([], [], []).size == 0
    finally:
        g.close()


# ---- the checks of the observed sweep

SIZES = (0, 1, 63, 64, 65, 255, 257, 5000)


def fold_once(new, off, hits, max_len=1000, max_blocks=0):
    f = new(max_len, max_blocks)
    try:
        f.add_hits(off, hits)
        return f.counts(), f.stat()
    finally:
        f.close()


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


def random_batch(world, n, max_len, seed):
    """gcb_cases' random units (all its categories), the fragments drawn shorter so that many keep both contexts on the transcript"""
    off, h = gc.random_batch(world, n, max_len, seed)
    rng = np.random.default_rng(seed + 1000)
    short = rng.integers(0, 2, h.size) == 1
    L = world["lens"][np.minimum(h["tid"], world["lens"].size - 1)]
    f = np.where(short & (L > 40) & (h["frag_len"] > 0) & (h["frag_len"] <= max_len), np.minimum(h["frag_len"], np.maximum(L // 4, 1)), h["frag_len"])
    h["frag_len"] = f.astype(np.uint32)
    inner = short & (L > 40) & (h["pos"] >= 0) & (h["pos"] <= h["mate_pos"])
    h["pos"] = np.where(inner, np.minimum(h["pos"], L // 2) + 3, h["pos"])
    h["mate_pos"] = np.where(inner, np.maximum(h["mate_pos"], h["pos"]), h["mate_pos"])
    return off, h


def check_sizes(world, new):
    for n in SIZES:
        off, h = random_batch(world, n, 1000, seed=100 + n)
        eo, es = check_against_restatement(world, new, off, h, what="%d units" % n)
        if n == 5000:
            assert es["used"] > 100 and es["overhang"] > 300 and all(es[k] > 0 for k in CATS[:7]), es
            assert np.count_nonzero(eo) > 300


def check_grid_caps(world, new):
    off, h = random_batch(world, 20001, 1000, seed=7)
    for mb in (1, 2, 0):
        check_against_restatement(world, new, off, h, max_blocks=mb, what="20 001 units, max_blocks %d" % mb)


def _one(tid, pos, mate_pos, frag_len):
    h = np.zeros(1, dtype=HIT_DTYPE)
    h["tid"] = tid; h["pos"] = pos; h["mate_pos"] = mate_pos; h["frag_len"] = frag_len; h["mate_status"] = 3; h["fwd"] = 1; h["mate_is_fwd"] = 0
    return h


def check_edges(world, new):
    """by hand, one by one: s = 2 | 3, s = L - 6 | L - 5, i = 4 | 5, i = L - 4 | L - 3, a fragment of one character, e = L | L + 1, tid = n_txps"""
    lens = [int(x) for x in world["lens"]]; T = len(lens)
    t = lens.index(1000); L = 1000
    assert (codes(world)[int(world["off"][t]): int(world["off"][t]) + L] < 4).all()
    for max_len in (1000, 40):
        f = min(30, max_len)
        rows = [  # (record, category)
            (_one(t, 2, 9, f), "overhang"), (_one(t, 3, 9, f), "used"), (_one(t, 9, 3, f), "used"), (_one(t, -4, 3, f), "overhang"),
            (_one(t, L - 6, L - 6, 3), "used"), (_one(t, L - 5, L - 5, 2), "overhang"),
            (_one(t, 3, 3, 2), "overhang"), (_one(t, 3, 3, 3), "used"),                        # i = 4 | 5
            (_one(t, L - 3 - f, L, f), "used"), (_one(t, L - 2 - f, L, f), "overhang"),        # i = L - 4 | L - 3
            (_one(t, 10, 10, 1), "used"),                                                     # both contexts on the same characters
            (_one(t, L - f, L, f), "overhang"), (_one(t, L + 1 - f, L, f), "overhang"),        # e = L | L + 1
            (_one(T, 10, 10, f), "overhang"), (_one(0xffffffff, 10, 10, f), "overhang"),
            (_one(lens.index(5000), 10, 10, max_len), "used"), (_one(t, 10, 10, max_len + 1), "out_of_range"), (_one(t, 10, 10, 0), "out_of_range"),
            (_one(lens.index(9), 3, 3, 1), "overhang"), (_one(lens.index(10), 3, 3, 3), "used"), (_one(lens.index(13), 3, 6, 6), "used"), (_one(lens.index(13), 3, 6, 7), "used"),
            (_one(lens.index(13), 3, 6, 8), "overhang"), (_one(lens.index(8), 3, 3, 3), "overhang"), (_one(lens.index(1), 0, 0, 1), "overhang"),
        ]
        h = np.concatenate([r[0] for r in rows]); off = np.arange(len(rows) + 1, dtype=np.int64)
        for i, (rec, cat) in enumerate(rows):
            o1, s1 = classify(world, [0, 1], rec, max_len)
            assert s1[cat] == 1, (i, cat, s1)                            # the restatement agrees with the hand
        eo, es = check_against_restatement(world, new, off, h, max_len=max_len, what="edges, max_len %d" % max_len)
        assert es["used"] == sum(1 for r in rows if r[1] == "used")


def check_multi_units(world, new):
    rng = np.random.default_rng(11)
    cats = np.array([gc.MULTI, gc.U, gc.MULTI, gc.MULTI, gc.UNM, gc.MULTI, gc.U] * 3)
    for sizes in ((2,), (3,), (200,), (2, 3, 200)):
        off, h = gc.build(world, cats, 1000, rng, multi_sizes=sizes)
        eo, es = check_against_restatement(world, new, off, h, what="units of %r hits" % (sizes,))
        assert es["multi"] == 12 and es["unmapped"] == 3 and es["used"] + es["overhang"] + es["ambiguous"] == 6


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
        assert es["out_of_range"] > 20 and es["used"] > 5


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
        # the counts bring their fragments only: `used` and the units grow by their number, the other categories stay where they were swept
        _, sa = classify(world, *a, 1000); _, sbb = classify(world, *b, 1000)
        assert so["used"] == sb_["used"] == sa["used"] + sbb["used"] and sbb["used"] > 20
        assert so["units"] == sa["units"] + sbb["used"] and sum(so[k] for k in CATS) == so["units"]
        for k in CATS[1:]:
            assert so[k] == sa[k] and sb_[k] == sa[k] + sbb[k]
    finally:
        both.close(); one.close(); other.close()


OBS_CHECKS = {f.__name__[6:]: f for f in (check_sizes, check_grid_caps, check_edges, check_multi_units, check_no_hits, check_max_lens,
                                          check_accumulate_and_clear, check_add_counts)}


# ---- the checks of the expected counts

def weight_sets(world, counts):
    """name -> q uint64[T]: all ones; zeros but a few; one huge q_t that takes the bound to just below 2^63"""
    T = world["lens"].size; lens = [int(x) for x in world["lens"]]
    Pm = prefix(counts)[-1]
    rng = np.random.default_rng(13)
    out = {"ones": np.ones(T, dtype=np.uint64), "zeros": np.zeros(T, dtype=np.uint64)}
    q = np.zeros(T, dtype=np.uint64); q[rng.integers(0, T, 4)] = rng.integers(1, 1000, 4).astype(np.uint64); out["sparse"] = q
    if Pm:
        q = np.ones(T, dtype=np.uint64); t = lens.index(1000)
        q[t] = np.uint64((2 ** 63 - 1 - (sum(lens) - lens[t]) * Pm) // (lens[t] * Pm))
        assert 2 ** 63 - lens[t] * Pm <= weight_bound(q, lens, counts) < 2 ** 63
        out["one huge"] = q
    return out


def _check_expect(world, new, max_len, max_blocks, names=None, sets=("ones", "zeros", "sparse", "one huge")):
    g = new(max_len, max_blocks)
    out = {}
    try:
        T = world["lens"].size
        for name, c in gc.histograms(world, max_len).items():
            if names is not None and name not in names:
                continue
            for qn, q in weight_sets(world, c).items():
                if qn not in sets:
                    continue
                ex = g.expect(c, T, q)
                exp, totals = expect(world, c, q)
                assert ex.dtype == np.uint64 and ex.shape == SHAPE
                assert np.array_equal(ex, exp), "%s, %s, max_len %d, max_blocks %d: differ at %r" % (name, qn, max_len, max_blocks, np.argwhere(ex != exp)[:5])
                assert_nine_sums(ex, totals, name)
                assert not ex[:, 0, 4:].any() and not ex[:, 1, 16:].any()
                out[(name, qn)] = ex
        return out
    finally:
        g.close()


def check_expect_default_grid(world, new):
    got = _check_expect(world, new, 1000, 0, sets=("ones", "zeros", "one huge"))
    assert not got[("empty", "ones")].any() and not got[("sparse", "zeros")].any() and got[("every length 1..300", "ones")][:, 2:].all()
    assert max(int(v.max()) for v in got.values()) > 2 ** 55 and len(got) >= 20


def check_expect_max_len_1(world, new):
    _check_expect(world, new, 1, 0)


def check_expect_max_len_1023(world, new):
    _check_expect(world, new, 1023, 0, names=("every length 1..300", "sparse", "counts near 2^32", "1, L, L + 1, max_len at L = 1000", "1, L, L + 1, max_len at L = 64"))


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
        off, h = random_batch(world, 300, 1000, seed=4)
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
        assert_nine_sums(ex, None, "just below the refusal")
        q[lens.index(1000)] += np.uint64(1)
        assert weight_bound(q, lens, c) >= 2 ** 63
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


# ---- the two host functions; weights_fn(alpha, lens, counts) and ratios_fn(obs, exp) are the implementations under test

def weight_inputs(T, seed, dominant=False, max_len=1000):
    rng = np.random.default_rng(seed)
    c = np.zeros(max_len + 1, dtype=np.uint64); c[150:450] = rng.integers(0, 5000, 300).astype(np.uint64)
    lens = rng.integers(1, 20000, T).astype(np.uint64); lens[: T // 10] = rng.integers(1, 400, T // 10)
    alpha = rng.random(T) * 100; alpha[rng.integers(0, T, T // 7)] = 0.0
    if dominant:
        alpha[:] = 1e-9; alpha[T // 2] = 1e12; lens[T // 2] = 180
    return alpha, lens, c


def check_weights(weights_fn):
    for T, seed, dom in ((2000, 71, False), (2000, 72, True), (1, 73, False), (300, 74, True)):
        alpha, lens, c = weight_inputs(T, seed, dom)
        if not dom:
            lens[0] = 700; alpha[0] = 3.5
        q, k = weights_fn(alpha, lens, c); eq, ek = weights(alpha, lens, c)
        assert k == ek and q.dtype == np.uint64 and np.array_equal(q, eq), (T, seed, k, ek)
        b = weight_bound(q, lens, c)
        assert 2 ** 59 < b < 2 ** 63, (T, seed, math.log2(b))        # the bound, and the weights keep next to all of the 62 bits
        assert (q[alpha == 0] == 0).all() and (q > 0).any()
    alpha, lens, c = weight_inputs(50, 75)
    for a, cc in ((np.zeros(50), c), (alpha, np.zeros_like(c)), (-alpha, c)):
        q, k = weights_fn(a, lens, cc)
        assert k == 0 and not q.any() and weights(a, lens, cc)[1] == 0
    short = lens.copy(); short[:] = 100                               # no fragment fits: S_t == 0 everywhere
    assert not weights_fn(alpha, short, c)[0].any()


def check_ratios(ratios_fn):
    rng = np.random.default_rng(81)
    obs = rng.integers(0, 100000, BINS).astype(np.uint64).reshape(SHAPE); ex = rng.integers(0, 1 << 50, BINS).astype(np.uint64).reshape(SHAPE)
    obs[0, 3, 8:12] = 0; ex[1, 4, 20:24] = 0                          # empty groups
    obs[0, 5, 0] = 10 ** 12; obs[0, 5, 1:4] = 1; ex[0, 5, 0] = 0; ex[0, 5, 1:4] = 10 ** 6   # ... and the clamps
    obs[1, 2, 60] = 0; obs[1, 2, 61:64] = 10 ** 9; ex[1, 2, 60:64] = 1000
    R = ratios_fn(obs, ex); E = ratios(obs, ex)
    assert R.dtype == np.float64 and R.shape == SHAPE and R.tobytes() == E.tobytes()
    assert (R[:, 0, 4:] == 1.0).all() and (R[:, 1, 16:] == 1.0).all() and R.min() == 0.25 and R.max() == 4.0
    assert R[0, 5, 0] == 4.0 and R[1, 2, 60] == 0.25 and (R[0, 3, 8:12] != 1.0).any()
    z = np.zeros(SHAPE, dtype=np.uint64)
    assert (ratios_fn(z, z) == 1.0).all()                             # nothing observed, nothing expected: (0 + 1) / (0 + 4) both ways


# ---- the checks of the effective lengths

def eff_histograms(max_len=1000):
    rng = np.random.default_rng(91)
    z = lambda: np.zeros(max_len + 1, dtype=np.uint64)
    out = {}
    a, b = (150, 451) if max_len >= 451 else (max_len // 5, max_len * 4 // 5 + 1)
    c = z(); c[a:b] = rng.integers(0, 5000, b - a).astype(np.uint64); c[1] = 3; c[9] = 1; c[max_len] = 7; out["a run's"] = c
    c = z(); c[rng.integers(1, max_len + 1, 12)] = rng.integers(1, 1 << 20, 12).astype(np.uint64); out["sparse"] = c
    return out


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
            assert e.tobytes() == fld_quotient(world, c).tobytes(), name
            if fld_fn is not None:
                assert np.allclose(e, fld_fn(c, world["lens"]), rtol=1e-12, atol=0)   # (L + 1) - Q / P: the same number by another formula
    finally:
        g.close()


def check_eff_exact_integers(world, new):
    """(b) R with entries 1 and 2 at one position per end, small counts: every partial sum is an integer below 2^53, so any order gives the same"""
    rng = np.random.default_rng(92)
    R = np.ones(SHAPE); R[0, 4, :] = rng.integers(1, 3, 64); R[1, 6, :] = rng.integers(1, 3, 64)
    c = np.zeros(1001, dtype=np.uint64); c[rng.integers(1, 1001, 40)] = rng.integers(1, 100, 40).astype(np.uint64); c[1] = 5
    g = new(1000, 0)
    try:
        e = g.eff_lens(c, world["lens"].size, R)
    finally:
        g.close()
    a = eff_lens(world, c, R, any_order=True); b = eff_lens(world, c, R)
    assert e.tobytes() == a.tobytes() == b.tobytes() and (e != fld_quotient(world, c)).any()


def check_eff_random(world, new):
    """(c) random R in [0.25, 4]: the restatement that spells out the tree, bit for bit; max_len 1000, 1023 and 100"""
    T = world["lens"].size
    for max_len in (1000, 1023, 100):
        g = new(max_len, 0)
        try:
            for i, (name, c) in enumerate(eff_histograms(max_len).items()):
                R = random_ratios(93 + i)
                e = g.eff_lens(c, T, R)
                assert e.tobytes() == eff_lens(world, c, R).tobytes(), (max_len, name)
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
    assert all(o.tobytes() == out[0].tobytes() for o in out) and out[0].tobytes() == eff_lens(world, c, R).tobytes()


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
    assert e.tobytes() == eff_lens(world, c, random_ratios(96)).tobytes()


EFF_CHECKS = {f.__name__[10:]: f for f in (check_eff_ratio_one, check_eff_exact_integers, check_eff_random, check_eff_grid_caps, check_eff_short_transcripts)}


def write_fasta(path, seqs):
    with open(path, "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b">t%d\n" % i + s + b"\n")


# ---- the planted bias: fragments thinned by the character they start with

PLANTED_SEED = 177
PLANTED_DRAWS = 16000
PLANTED_KEEP = (0.25, 0.25, 1.0, 0.25)                               # the probability to keep a fragment whose first character is A, C, G, T


def _mix_seq(rng, n, g):
    """n characters, each G with probability g, else A, C or T alike"""
    p = np.array([(1 - g) / 3, (1 - g) / 3, g, (1 - g) / 3])
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.choice(4, size=n, p=p)]


def planted_transcripts(seed=PLANTED_SEED):
    """-> (names, transcripts uint8, abundances).  40 transcripts of their own, each of three stretches of 500 characters with 10 %, 25 % and
    40 % G in random order: they map uniquely, and since each holds starts of every kind, what is observed along ONE transcript shows the
    bias whatever that transcript's abundance.  10 genes of two isoforms: 450 shared characters at 25 % G and 650 of the isoform's own,
    in which the favoured start -- a fragment that begins with G -- is four times as frequent in one isoform (40 %) as in the other
    (10 %); the shared part in front in every other gene.  A fragment of the shared part maps to both isoforms: how the estimate splits
    those is what the effective lengths decide, so that is where the bias shows in NumReads."""
    rng = np.random.default_rng(seed)
    names, txps = [], []
    for i in range(40):
        g = np.array([0.1, 0.25, 0.4])[rng.permutation(3)]
        names.append("S%d" % i); txps.append(np.concatenate([_mix_seq(rng, 500, x) for x in g]))
    for gene in range(10):
        shared = _mix_seq(rng, 450, 0.25)
        for iso, g in (("A", 0.4), ("B", 0.1)):
            own = _mix_seq(rng, 650, g)
            names.append("G%d.%s" % (gene, iso)); txps.append(np.concatenate([shared, own] if gene % 2 == 0 else [own, shared]))
    theta = rng.uniform(0.5, 2.0, len(txps))
    return names, txps, theta


def planted_fragments(txps, theta, n_draws=PLANTED_DRAWS, seed=PLANTED_SEED + 1, read_len=60):
    """n_draws fragments: a transcript by abundance x length, a length of N(220, 20) clipped to [150, 300], a start uniform over the
    transcript; each kept with PLANTED_KEEP of its first character.  -> (reads1, reads2 as lists of bytes, mate 2 reverse-complemented,
    the mates swapped in half of the pairs; tid int64[kept] of the transcript each kept fragment came from)"""
    from rapmap_amd.synth import _COMP
    rng = np.random.default_rng(seed)
    lens = np.array([t.size for t in txps], dtype=np.int64)
    w = theta * lens
    tid = rng.choice(len(txps), size=n_draws, p=w / w.sum())
    flen = np.clip(rng.normal(220, 20, n_draws).astype(np.int64), 150, 300)
    start = (rng.random(n_draws) * (lens[tid] - flen + 1)).astype(np.int64)
    u = rng.random(n_draws); swap = rng.random(n_draws) < 0.5
    r1, r2, origin = [], [], []
    for i in range(n_draws):
        f = txps[int(tid[i])][int(start[i]):int(start[i] + flen[i])]
        if u[i] >= PLANTED_KEEP[int(_CODE[f[0]])]:
            continue
        a = f[:read_len].tobytes(); b = _COMP[f[::-1][:read_len]].tobytes()
        if swap[i]:
            a, b = b, a
        r1.append(a); r2.append(b); origin.append(int(tid[i]))
    return r1, r2, np.array(origin, dtype=np.int64)
