"""Transcripts that hold the same k-mer more than once -- tandem arrays, a segment dispersed through a transcript, inverted repeats: data
and checks of test_txp_repeats.py (the lane emulation of the device source) and test_txp_repeats_gpu.py (the HIP path).  Every other
fixture of the suite lists a transcript at most once in any suffix-array interval (conftest's repeat_data puts every copy of a core into
a transcript of its own; synth.make_transcriptome shares exons between transcripts, never within one), so the rule "one position per
transcript, the smallest signed pos - queryPos" (HitManager.cpp:761-767, :309-313) has two candidates to choose between here only.

The reference is the oracle (oracle.Oracle(q5.load(idx))); truth_check() is the one check that goes neither through the oracle nor
through the suffix array.  reach() is a condition on the DATA, asked of the oracle's own hits and intervals.

The seeds: txome(k, seed=TXOME_SEED) -- make_transcriptome(6, seed) for the ordinary genes, default_rng(seed * 1000 + k) for everything
else; reads(..., seed=READS_SEED) -- default_rng(seed * 1000 + L * 32 + k) for overhangs and paddings.  Nothing else is random.

No test functions here.  Indices and read sets are built once per process (mapping_harness.once)."""
import re

import numpy as np

import mapping_harness as mh

TXOME_SEED = 53
READS_SEED = 11

# Reads the pair and the lean kernel leave to the general kernel on reads_for(k, 100) under default options, and how many of the reads
# they KEEP have their hit list from one interval that lists a transcript more than once (so their per-transcript minimum decided
# something).  From the lane emulation (QM_EMU_LEAN_STATS=2); test_txp_repeats_gpu.py holds qm_ctx_stat(QM_STAT_LEAN_DEFERRED) to
# "pair" / "lean".
EXPECT_LEFT = {
    (31, "dense"): {"pair": 2777, "lean": 1816, "pair_kept_repeated": 759, "lean_kept_repeated": 1582},
    (31, "ph_compact"): {"pair": 2777, "lean": 1816, "pair_kept_repeated": 759, "lean_kept_repeated": 1582},
    (21, "dense"): {"pair": 2976, "lean": 1944, "pair_kept_repeated": 720, "lean_kept_repeated": 1558},
    (15, "dense"): {"pair": 3300, "lean": 2247, "pair_kept_repeated": 613, "lean_kept_repeated": 1453},
}

COPIES = (2, 3, 8, 9, 33, 63, 64, 65, 70, 130)      # either side of 8 (a byte of lanes), 32, 64 (a wavefront) and of 64 NS - P at NS = 3
MAX_ARRAY = 9000                                    # characters: a (unit, copies) beyond it is left out
LONG_UNIT, LONG_COPIES = 40, (900, 1100)            # either side of max_interval = 1000 inside ONE transcript
SEG, SEG_COPIES = 120, (1, 2, 3, 5, 70)             # one interval of the segment: 81 suffixes over five transcripts


def units(k):
    return (2, 3, 7, k - 1, k, k + 1, 45, 100, 130)


def pfcap(ns, L, k):
    """how many (tid, pos) records of a strand's first interval the general kernel stages in LDS (qm_mapper.inl, collect_read): the slots
    of the interval table behind the read's last k-mer"""
    return 64 * ns - (L - k + 1)


def rc(a):
    return mh.COMP[a[::-1]]


def _primitive(u):
    b = u.tobytes()
    return (b + b).find(b, 1) == len(b)


def txome(k, seed=TXOME_SEED):
    """-> {"names", "seqs" (uint8 arrays, file order), "arrays": [(transcript, start of the array, unit length, copies)], "inverted":
    the transcripts that hold a segment and its reverse complement, "walked": the transcripts that reads() walks end to end}.
    6 ordinary genes; for every unit length of units(k) and every copy number of COPIES a tandem array of a random unit (no power of a
    shorter word, nor its own reverse complement read round the array) three times: between flanks of 120 random characters, at the very start of a transcript, at its very end; 900 and 1 100
    copies of a 40-mer; one 120-mer 1, 2, 3, 5 and 70 times in five transcripts between spacers of 20 .. 200 characters; two inverted
    repeats."""
    def make():
        from rapmap_amd import synth
        rng = np.random.default_rng(seed * 1000 + k)
        rand = lambda n: mh.ACGT[rng.integers(0, 4, n)]

        def unit(n):
            u = rand(n)
            while not _primitive(u) or rc(u).tobytes() in 2 * u.tobytes():     # (AT, ACGT, ...: an array that is its own reverse complement)
                u = rand(n)
            return u
        gn, gs = synth.make_transcriptome(6, seed)
        first = {}
        for i, t in enumerate(gs):
            first.setdefault(t.tobytes(), i)
        names, seqs = [gn[i] for i in sorted(first.values())], [gs[i] for i in sorted(first.values())]
        ngenes = len(seqs)
        arrays, inverted, walked = [], [], []

        def add(name, parts):
            names.append(name); seqs.append(np.concatenate(parts))
            return len(seqs) - 1
        for U in units(k):
            for c in COPIES:
                if U * c > MAX_ARRAY:
                    continue
                for where in ("mid", "start", "end"):
                    u = unit(U)                      # (one per transcript: only the 2- and 3-mers meet again in other transcripts, by chance)
                    l, r = rand(0 if where == "start" else 120), rand(0 if where == "end" else 120)
                    arrays.append((add("tand_U%d_c%d_%s" % (U, c, where), [l] + [u] * c + [r]), l.size, U, c))
        for c in LONG_COPIES:
            l = rand(120)
            arrays.append((add("tand_U%d_c%d_mid" % (LONG_UNIT, c), [l] + [unit(LONG_UNIT)] * c + [rand(120)]), l.size, LONG_UNIT, c))
        seg = rand(SEG)
        for m in SEG_COPIES:
            parts = []
            for _ in range(m):
                parts += [rand(int(rng.integers(20, 201))), seg]
            walked.append(add("disp_%d" % m, parts + [rand(60)]))
        for j in range(2):
            s = rand(150 + 30 * j)
            inverted.append(add("inv_%d" % j, [rand(80), s, rand(90 - 60 * j), rc(s), rand(70)]))
        walked += inverted
        assert len({s.tobytes() for s in seqs}) == len(seqs), "two equal transcripts: the indexer would drop one"
        return {"names": names, "seqs": seqs, "arrays": arrays, "inverted": set(inverted), "walked": walked, "genes": list(range(ngenes))}
    return mh.once(("repeat_txome", k, seed), make)


def index_for(tmp_root, k, image, seed=TXOME_SEED):
    """txome(k) indexed at k; image: "dense" or "ph" (`quasiindex -p`).  The index holds every transcript, in file order."""
    def make():
        tx = txome(k, seed)
        return mh.index_of(tmp_root, "repeats", k, image, tx["names"], tx["seqs"])
    return mh.once(("repeat_index", k, image, seed), make)


def reads(tx, L, k, seed=READS_SEED):
    """-> (reads1, reads2, truth): pairs of up to 2 x L characters.  Mate 1 of every array (t, st, U, c) starts 40 and 5 before the array,
    at it, 1, U - 1 and U inside it, 3 behind the middle copy's start, so that it ends 10 behind the array (array into flank), exactly at
    the array's last copy, and 20 before the array's end (flank or the transcript's end inside the read: behind the transcript's end the
    read goes on with random characters); on the arrays at a transcript's start also 3 and 30 BEFORE the transcript (random characters,
    then the transcript: the first copy has a negative position, every later one a positive one).  Mate 2 is the reverse complement of
    the window 60 further on (pulled back inside the transcript), so the two mates favour different copies.  The transcripts of
    tx["walked"] and the genes are walked end to end in steps of 37 and of 211.  Pair i: i % 4 == 1 -- one substitution in the middle of
    mate 1 (two MMPs); 2 -- the mates swapped; 3 -- both reverse-complemented.
    truth[i] = the two mates as they stand in reads1[i], reads2[i]: (transcript, forward?, edited?, characters in front of the transcript's
    start)."""
    rng = np.random.default_rng(seed * 1000 + L * 32 + k)
    rand = lambda n: mh.ACGT[rng.integers(0, 4, n)]
    seqs = tx["seqs"]
    r1, r2, truth = [], [], []

    def pair(t, a, over, b0):
        T = seqs[t]
        b = T[b0:b0 + L]
        if a.size < k or b.size < k:
            return
        a = a.copy(); b = rc(b)
        ea, eb = [t, True, False, over], [t, False, False, 0]
        kind = len(r1) % 4
        if kind == 1:
            a[a.size // 2] = mh.ACGT[(np.searchsorted(mh.ACGT, a[a.size // 2]) + 1) % 4]
            ea[2] = True
        if kind == 2:
            a, b, ea, eb = b, a, eb, ea
        if kind == 3:
            a, b = rc(a), rc(b)
            ea[1], eb[1] = not ea[1], not eb[1]
        r1.append(a.tobytes()); r2.append(b.tobytes()); truth.append((tuple(ea), tuple(eb)))

    for (t, st, U, c) in tx["arrays"]:
        T = seqs[t]
        end = st + U * c
        for a0 in sorted({st - 40, st - 5, st, st + 1, st + U - 1, st + U, st + (c // 2) * U + 3, end - L + 10, end - L, end - 20, -30, -3}):
            if a0 < 0:
                if st != 0 or a0 not in (-30, -3):
                    continue
                a = np.concatenate([rand(-a0), T[:L + a0]])
            else:
                a = T[a0:a0 + L]
                if k <= a.size < L:
                    a = np.concatenate([a, rand(L - a.size)])
            pair(t, a, max(0, -a0), min(max(0, a0) + 60, max(0, T.size - L)))
    for step, which in ((37, tx["walked"]), (211, tx["genes"])):
        for t in which:
            T = seqs[t]
            for a0 in range(0, max(1, T.size - L), step):
                pair(t, T[a0:a0 + L], 0, min(a0 + 90, max(0, T.size - L)))
    return r1, r2, truth


def reads_for(k, L, seed=READS_SEED):
    """reads() over txome(k), packed: -> {"r1", "r2", "truth", "q1", "o1", "q2", "o2", "n", "lens" (of the transcripts)}"""
    def make():
        from util import pack
        tx = txome(k)
        r1, r2, truth = reads(tx, L, k, seed)
        q1, o1 = pack(r1); q2, o2 = pack(r2)
        assert max(np.diff(o1).max(), np.diff(o2).max()) == L
        return {"r1": r1, "r2": r2, "truth": truth, "q1": q1, "o1": o1, "q2": q2, "o2": o2, "n": len(r1), "lens": np.array([s.size for s in tx["seqs"]], dtype=np.int64)}
    return mh.once(("repeat_reads_for", k, L, seed), make)


def n_reads(k, L, every=23):
    """every 23rd pair of reads_for(k, L) with an N in the middle of mate 1 and at a third of mate 2: most of them inside an array (the
    N-aware second pass of the lean kernel).  -> (reads1, reads2)"""
    def make():
        rd = reads_for(k, L)
        r1, r2 = [], []
        for i in range(0, rd["n"], every):
            a, b = bytearray(rd["r1"][i]), bytearray(rd["r2"][i])
            a[len(a) // 2] = ord("N"); b[len(b) // 3] = ord("N")
            r1.append(bytes(a)); r2.append(bytes(b))
        return r1, r2
    return mh.once(("repeat_n_reads", k, L, every), make)


def mixed(k, L, extra):
    """reads_for(k, L) and one pair of `extra` characters behind them (100 before the 900-copy array and into it, mate 2 60 further on),
    packed: (q1, o1, q2, o2).  The longest read of a batch picks the slot class of the whole batch (qm_host.hip, map_device_impl)."""
    def make():
        from util import pack
        tx, rd = txome(k), reads_for(k, L)
        t, st, U, c = [a for a in tx["arrays"] if a[3] == LONG_COPIES[0]][0]
        T = tx["seqs"][t]
        a, b = T[st - 100:st - 100 + extra], rc(T[st - 40:st - 40 + extra])
        assert a.size == extra and b.size == extra
        return pack(rd["r1"] + [a.tobytes()]) + pack(rd["r2"] + [b.tobytes()])
    return mh.once(("repeat_mixed", k, L, extra), make)


def single_truth(truth):
    """the truth entries of mh.odd_single(reads1, reads2)"""
    one = [a for a, b in truth[:-1]] + [truth[1][1]]
    return one[:-1] if len(one) % 2 == 0 else one


# ---- the checks

def sa_tids(ix):
    """the transcript of every suffix-array entry of an index as the oracle reads it (q5.load)"""
    return np.searchsorted(np.asarray(ix.txpOffsets, dtype=np.int64), np.asarray(ix.SA, dtype=np.int64), side="right") - 1


def repeated(ix, ints):
    """per interval record (oracle: res.ints): does its suffix-array range list a transcript more than once?"""
    tid = sa_tids(ix)
    memo, out = {}, np.zeros(len(ints), dtype=bool)
    for j, (b, e) in enumerate(zip(ints[:, 0].tolist(), ints[:, 1].tolist())):
        if (b, e) not in memo:
            memo[(b, e)] = np.unique(tid[b:e]).size < e - b
        out[j] = memo[(b, e)]
    return out


# reach()'s counts on the oracle's results per (k, read length), dense image (pinned: the data may not drift):
# negative positions among single-end records and among the orphans of the paired call; intervals of the paired call under
# maxInterval = 100 000 that list a transcript more than once, by width: at most 64, 65 .. pfcap(3, L, k), above it; those of 50 and
# more suffixes and of 1 000 and more (what maxInterval 50 and 1000 drop).  Filled in from the oracle, never from the code under test.
REACH = {(31, 100): (167, 3, 2647, 654, 389, 2248, 15), (21, 100): (147, 4, 2452, 699, 415, 2207, 15), (15, 100): (169, 3, 2708, 469, 575, 2257, 16),
         (31, 150): (185, 3, 2421, 270, 524, 1778, 15), (31, 250): (205, 12, 2105, 0, 2592, 1534, 15)}


def reach(ix, orc, oracle_mod, rd, L, k):
    """-> the tuple that REACH pins, asked of the ORACLE alone"""
    from util import pack
    q, o = pack(mh.odd_single(rd["r1"], rd["r2"]))
    rs = orc.map_single(q, o, nthreads=4)
    rp = orc.map_pairs(rd["q1"], rd["o1"], rd["q2"], rd["o2"], nthreads=4)
    orphans = rp.hits[rp.hits["mate_status"] != 3]
    wide = orc.map_pairs(rd["q1"], rd["o1"], rd["q2"], rd["o2"], opts=oracle_mod.default_opts(maxInterval=100000), nthreads=4, want_ints=True)
    w = (wide.ints[:, 1] - wide.ints[:, 0]).astype(np.int64)
    rep = repeated(ix, wide.ints)
    cap = pfcap(3, L, k)
    return (int((rs.hits["pos"] < 0).sum()), int((orphans["pos"] < 0).sum()), int((rep & (w <= 64)).sum()), int((rep & (w > 64) & (w <= cap)).sum()),
            int((rep & (w > cap)).sum()), int((w >= 50).sum()), int((w >= 1000).sum()))


def assert_reach(got, what, cap):
    """cap: pfcap(3, L, k) -- where it is 64 or less (reads beyond 160 characters) no interval is staged beyond a wavefront's lanes"""
    neg_single, neg_orphan, small, staged, large, over50, over1000 = got
    assert neg_single + neg_orphan >= 100, (what, got)
    assert small > 0 and (staged > 0 or cap <= 64) and large > 0, (what, got)
    assert over50 > 0 and over1000 > 0, (what, got)


def reads_with_repeated_interval(ix, res):
    """per read (2 u + mate) of a paired oracle result mapped with want_ints=True: True where the read has exactly one interval on a
    strand -- the case in which its hit list comes from that interval alone -- and that interval lists a transcript more than once"""
    rep = repeated(ix, res.ints)
    n = len(res.ints_offsets) - 1
    out = np.zeros(2 * n, dtype=bool)
    lst = res.ints[:, 5]
    for u in range(n):
        a, b = int(res.ints_offsets[u]), int(res.ints_offsets[u + 1])
        for l in range(4):
            sel = np.nonzero(lst[a:b] == l)[0]
            if sel.size == 1 and rep[a + sel[0]]:
                out[2 * u + (l >> 1)] = True
    return out


def emu_left_reads(err_text):
    """{"pair": set of the reads the pair kernel left in its fused pass, "lean": ... the lean kernel left after both passes} from the lines
    the emulation prints under QM_EMU_LEAN_STATS=2"""
    out = {}
    for name, pat in (("pair", r"pair kernel \(pass 0\) left:([ \d]*)"), ("lean", r"lean kernel left:([ \d]*)")):
        m = re.search(pat, err_text)
        if m:
            out[name] = {int(x) for x in m.group(1).split()}
    return out


MAX_INTERVAL = 1000


def _count(T, r, limit):
    """occurrences of r in T, overlapping ones too, counted up to limit"""
    n, p = 0, T.find(r)
    while p >= 0 and n < limit:
        n += 1
        p = T.find(r, p + 1)
    return n


def expected(tx, e, r, k):
    """one mate `r` with truth entry `e` -> None (not eligible), or (position, why it is left out or None).
    Eligible: no edit, not from a transcript of tx["inverted"], and the characters inside the transcript T (all but the `over` in front of
    its start, in T's orientation) occur verbatim in T.
    The rule: the collector looks the read's k-mers up from its first on until one is in the index (SACollector.hpp:167-237), at j,
    then takes the maximal match from there.  Where the read from j on occurs in T, that match runs to the read's end, the read has ONE
    interval -- the suffixes that start with those characters -- and collectFromSingleInterval keeps per transcript the smallest
    pos - queryPos (HitManager.cpp:761-767): the position is (the LEFTMOST place bytes.find finds read[j:] in T) - j.  For a read inside
    its transcript j is 0.  For a read that hangs over T's start by `over` random characters j is `over` -- unless those characters happen
    to go on as the text in front of some copy does (an array of 2-, 3- or 7-mers: one chance in 4 per character), when an earlier k-mer
    is found: j is then the first place whose k-mer occurs anywhere in the transcriptome, on either strand.
    Left out, each from the sequences alone:
    "elsewhere" -- the read from that j on does not occur in T (the first k-mer found is another transcript's, or lies on T's other
      strand: the match from there ends early or on an interval without T, and what follows is intersectSAHits over several intervals,
      not this rule);
    "max_interval" -- read[j:] occurs MAX_INTERVAL times or more in T (the 1 100-copy array): the collector drops an interval of
      maxInterval suffixes or more (SACollector.hpp:577), and the read maps through what is left or not at all."""
    ti, fwd, edited, over = e
    if edited or ti in tx["inverted"]:
        return None
    T = tx["seqs"][ti].tobytes()
    w = np.frombuffer(r, dtype=np.uint8)
    w = (w if fwd else rc(w)).tobytes()
    if T.find(w[over:]) < 0:
        return None
    j = 0
    if over:
        j = int(np.argmax(_among(_tables(tx, k)[0], _codes(np.frombuffer(w, dtype=np.uint8), k))))    # (the k-mers at `over` and behind are T's)
    p = T.find(w[j:])
    if p < 0:
        return -over, "elsewhere"
    if _count(T, w[j:], MAX_INTERVAL) >= MAX_INTERVAL:
        return p - j, "max_interval"
    return p - j, None


def _codes(a, k):
    """the k-mers of a string of A C G T as 2 k-bit numbers"""
    v = np.searchsorted(mh.ACGT, a).astype(np.uint64)
    n = a.size - k + 1
    c = np.zeros(max(n, 0), dtype=np.uint64)
    for j in range(k if n > 0 else 0):
        c = (c << np.uint64(2)) | v[j:j + n]
    return c


def _tables(tx, k):
    """(the k-mers that occur in the transcriptome on either strand, those of them that occur in more than one transcript), sorted"""
    if ("kmers", k) not in tx:
        c = np.concatenate([_codes(x, k) for s in tx["seqs"] for x in (s, rc(s))])
        t = np.concatenate([np.full(2 * max(s.size - k + 1, 0), i) for i, s in enumerate(tx["seqs"])])
        o = np.lexsort((t, c))
        c, t = c[o], t[o]
        first = np.append(True, (c[1:] != c[:-1]) | (t[1:] != t[:-1]))
        u = c[first]
        tx[("kmers", k)] = (np.unique(u), np.unique(u[1:][u[1:] == u[:-1]]))
    return tx[("kmers", k)]


def _among(table, codes):
    """per code: is it in the sorted table?"""
    i = np.minimum(np.searchsorted(table, codes), table.size - 1)
    return table[i] == codes


def shared(tx, e, r, k):
    """does a k-mer of this mate occur in another transcript than its own as well, on either strand?  (arrays of the same 2- or 3-mer or
    of its reverse complement, the dispersed segment, exons of a gene)"""
    return bool(_among(_tables(tx, k)[1], _codes(np.frombuffer(r, dtype=np.uint8), k)).any())


def hits_its_transcript(tx, e, r, x, k):
    """may truth_check count on this mate to have its transcript T among its hits?  x = expected(tx, e, r, k).  Yes for a mate under
    the rule, and for a mate inside T with one substitution in its middle whose two halves lie in T at places that fit, as long as no
    k-mer that holds the substituted character occurs anywhere (a G put into a CT array makes ...CTG TCTC..., and another transcript's
    flank may end in G in front of its TC array: a third maximal match, on an interval without T)."""
    if x is not None:
        return x[1] is None
    ti, fwd, edited, over = e
    if not edited or over or ti in tx["inverted"]:
        return False
    T = tx["seqs"][ti].tobytes()
    w = np.frombuffer(r, dtype=np.uint8)
    w = (w if fwd else rc(w)).tobytes()
    h = len(w) // 2                                         # (reads() edits mate 1 as cut, forward, in its middle)
    assert fwd
    if _among(_tables(tx, k)[0], _codes(np.frombuffer(w, dtype=np.uint8)[max(0, h - k + 1):h + k], k)).any():
        return False
    p = T.find(w[:h])
    while p >= 0:
        if T[p + h + 1:p + len(w)] == w[h + 1:]:
            return True
        p = T.find(w[:h], p + 1)
    return False


def truth_check(hit_offsets, hits, rd, tx, k, single=False, min_checked=1000, min_negative=20):
    """Every eligible mate that expected() does not leave out has its transcript T among its unit's hits, on the strand it was cut from, at
    the position expected() works out with bytes.find.  Nothing here goes through the oracle or the suffix array.  Single-end units and
    orphans hold the position itself; paired units: mate 1 is `pos` / `fwd` of a record that is paired or a left orphan, mate 2 is
    `mate_pos` / `mate_is_fwd` of a paired record or `pos` / `fwd` of a right orphan, and a paired record holds max(position, 0)
    (ends_cases.truth_check).  In a pair, a mate is left out as well ("other mate") when the OTHER mate cannot be counted on to hit
    T (hits_its_transcript()) and a k-mer of this mate occurs in another transcript too (shared()): the other mate may then
    miss T, the pair joins on the other transcripts alone, and a unit with paired records reports no orphans.
    At most 5 % of the eligible mates may be left out.  -> (eligible mates, checked, of them at a negative position, {why: left out})"""
    hits = np.asarray(hits)
    truth = rd["truth"]
    units = [(i, (e,), (r,)) for i, (e, r) in enumerate(zip(single_truth(truth), mh.odd_single(rd["r1"], rd["r2"])))] if single else \
        [(i, truth[i], (rd["r1"][i], rd["r2"][i])) for i in range(rd["n"])]
    eligible = checked = negative = 0
    out, missing = {}, []
    for i, mates, rr in units:
        h = hits[hit_offsets[i]:hit_offsets[i + 1]]
        exp = [expected(tx, e, r, k) for e, r in zip(mates, rr)]
        for m, (e, x) in enumerate(zip(mates, exp)):
            if x is None:
                continue
            eligible += 1
            p, why = x
            if why is None and not single and not hits_its_transcript(tx, mates[1 - m], rr[1 - m], exp[1 - m], k) and shared(tx, e, rr[m], k):
                why = "other mate"
            if why is not None:
                out[why] = out.get(why, 0) + 1
                continue
            ti, fwd = e[0], e[1]
            own = h[h["tid"] == ti]
            if single:
                ok = ((own["pos"] == p) & (own["fwd"] == fwd)).any()
            elif m == 0:
                ok = ((own["fwd"] == fwd) & (((own["pos"] == max(p, 0)) & (own["mate_status"] == 3)) | ((own["pos"] == p) & (own["mate_status"] == 1)))).any()
            else:
                ok = (((own["mate_pos"] == max(p, 0)) & (own["mate_is_fwd"] == fwd) & (own["mate_status"] == 3)) |
                      ((own["pos"] == p) & (own["fwd"] == fwd) & (own["mate_status"] == 2))).any()
            checked += 1
            negative += p < 0
            if not ok:
                missing.append((i, m, e, p))
    assert not missing, "%d of %d mates lack their own transcript, strand and leftmost position among their unit's hits, first (unit, mate, truth, position): %r" % (
        len(missing), checked, missing[:5])
    assert eligible - checked <= 0.05 * eligible, "%d of %d eligible mates left out (%r): more than 5 %%" % (eligible - checked, eligible, out)
    assert checked >= min_checked and negative >= min_negative, (checked, negative)
    return eligible, checked, negative, out


# ---- the option sets (mapping_harness.OPTION_SETS)

VARIANTS = ("default", "noStrictCheck", "fuzzy", "fuzzy_noDovetail", "noSensitive", "noDovetail", "noOrphans", "m3", "maxInterval50", "z0.9", "selAln",
            "selAln_hardFilter", "mimicBT2", "mimicStrictBT2")
FEW = ("default", "fuzzy", "maxInterval50", "selAln")
