"""Transcripts shorter than a read and reads that hang over a transcript end: data and checks of test_txp_ends.py (the lane emulation of
the device source) and test_txp_ends_gpu.py (the HIP path).  Every other fixture of the suite has transcripts of 200 characters or more
and reads that lie inside them (at most flush with an end), so negative positions, targets shorter than the query and a `$` or the end
of the text right behind a k-mer are met here only.

The reference is the oracle (oracle.Oracle(q5.load(idx))); truth_check() is the one check that goes neither through the oracle nor
through the suffix array.  reach() is a condition on the DATA: every test that maps asserts its minimums on the oracle's own result, so
the reads cannot drift away from the edges unnoticed.

The seeds: txome(k, seed=TXOME_SEED) -- make_transcriptome(8, seed) for the ordinary genes, default_rng(seed * 1000 + k) for the random
transcripts and the places of the substrings; reads(..., seed=READS_SEED) -- default_rng(seed * 1000 + L * 32 + k) for flanks and
substitutions.  Nothing else is random.

No test functions here.  Indices and read sets are built once per process (mapping_harness.once)."""
import numpy as np

import mapping_harness as mh

TXOME_SEED = 31
READS_SEED = 7

# the minimums of reach() on the oracle's hits, per option set: (pos < 0, pos + L > transcript length, transcript shorter than L)
REACH_DEFAULT = (100, 1000, 100)
REACH_SEL_NEGATIVE = 100


def random_lengths(k):
    return [1, 5, k - 1, k, k + 1, 2 * k - 1, 2 * k, 63, 64, 65, 99, 100, 101, 127, 128, 129, 150]


def txome(k, seed=TXOME_SEED):
    """-> (names, sequences as uint8 arrays), in file order: one transcript of k - 1 characters (the text begins with a transcript that
    has no k-mer); 8 ordinary genes; random transcripts of random_lengths(k); exact substrings of ordinary transcripts (60 from the middle
    of one, the first 80 of another, the last 80 of a third, exactly k and k + 1 from the middle of two more, 100 and 130 from the middle
    of another); a second set of the random lengths; last a transcript of exactly k characters (one k-mer, then the final `$`).  No two
    are equal (the indexer removes exact duplicates: the 1- and 5-character ones of the two sets are made to differ)."""
    def make():
        from rapmap_amd import synth
        rng = np.random.default_rng(seed * 1000 + k)
        rand = lambda n: mh.ACGT[rng.integers(0, 4, n)]
        names, seqs = ["first_k-1"], [rand(k - 1)]
        gn, gs = synth.make_transcriptome(8, seed)
        first = {}
        for i, t in enumerate(gs):                                              # (two isoforms that keep the same exons are one transcript)
            first.setdefault(t.tobytes(), i)
        gn, gs = [gn[i] for i in sorted(first.values())], [gs[i] for i in sorted(first.values())]
        assert len(gs) >= 8 and min(t.size for t in gs) >= 300
        names += gn; seqs += gs

        def random_set(tag):
            for n in random_lengths(k):
                t = rand(n)
                while any(t.size == s.size and t.tobytes() == s.tobytes() for s in seqs):
                    t = mh.ACGT[(np.searchsorted(mh.ACGT, t) + 1) % 4]                    # (a 1-character transcript has four values)
                names.append("%s_%d" % (tag, n)); seqs.append(t)
        random_set("rnd")
        src = [gs[i] for i in rng.permutation(len(gs))[:6]]
        mid = lambda t, n: t[(t.size - n) // 2:(t.size - n) // 2 + n].copy()
        for nm, t in (("sub_mid60", mid(src[0], 60)), ("sub_first80", src[1][:80].copy()), ("sub_last80", src[2][-80:].copy()), ("sub_k", mid(src[3], k)),
                      ("sub_k+1", mid(src[4], k + 1)), ("sub_mid100", mid(src[5], 100)), ("sub_mid130", mid(src[5], 130))):
            names.append(nm); seqs.append(t)
        random_set("rnd2")
        names.append("last_k"); seqs.append(rand(k))
        assert len({s.tobytes() for s in seqs}) == len(seqs), "two equal transcripts: the indexer would drop one"
        return names, seqs
    return mh.once(("ends_txome", k, seed), make)


def index_for(tmp_root, k, image, seed=TXOME_SEED):
    """txome(k) indexed at k; image: "dense" or "ph" (`quasiindex -p`).  The index holds every transcript, in file order."""
    return mh.once(("ends_index", k, image, seed), lambda: mh.index_of(tmp_root, "ends", k, image, *txome(k, seed)))


def overhangs(L, k):
    """by how many characters mate 1 hangs over an end; the last four leave k + 1, k, k - 1 and 1 characters inside"""
    return sorted({0, 1, 2, 7, 8, 9, 20, L - k - 1, L - k, L - k + 1, L - 1})


def reads(txps, L, k, seed=READS_SEED):
    """-> (reads1, reads2, truth): pairs of 2 x L characters.  Every transcript t is taken twice: between flanks of random characters, and
    between flanks taken from the transcripts before and behind it in the file (so a read holds the end of one transcript and the start of
    the next without the `$`).  Mate 1 is cut from flank + t + flank at starts that hang over the left end, and over the right end, by
    every d of overhangs(L, k); for a t shorter than L also with t slid through the read in six steps.  Mate 2 is the reverse complement
    of, in turn: the same window (full overlap), the window 30 to the left (a dovetail), the window 50 to the right, the window that ends
    10 behind t's right end.  One read in seven has a substitution in the middle, one in eleven a one-base deletion there (the next
    character of the flank keeps its length); half the pairs (four in every eight) have their mates swapped.
    truth[i] = the two mates of pair i as they stand in reads1[i], reads2[i]: (transcript, start in it -- negative for a left overhang --,
    forward?, edited?, random flanks?, characters inside the transcript, runs on?).  runs on: t lies inside another transcript u as well, and
    the read's character right in front of t or right behind it is u's: a maximal match from inside t runs on into u and so ends on an
    interval without t (see truth_check)."""
    rng = np.random.default_rng(seed * 1000 + L * 32 + k)
    F = L + 60                                                          # every window below lies inside flank + t + flank
    r1, r2, truth = [], [], []
    nread = 0
    whole = [t.tobytes() for t in txps]
    for ti, t in enumerate(txps):
        T = t.size
        inside_of = []                                                  # (u, where t lies in u), asked only of a t that truth_check can cover
        for ui, u in enumerate(whole if T >= 2 * k else []):
            o = u.find(whole[ti]) if ui != ti else -1
            while o >= 0:
                inside_of.append((txps[ui], o))
                o = u.find(whole[ti], o + 1)
        for random_flanks in (True, False):
            if random_flanks:
                fl, fr = mh.ACGT[rng.integers(0, 4, F)], mh.ACGT[rng.integers(0, 4, F)]
            else:
                before = np.concatenate([mh.ACGT[rng.integers(0, 4, F)]] + list(txps[:ti]))
                behind = np.concatenate(list(txps[ti + 1:]) + [mh.ACGT[rng.integers(0, 4, F)]])
                fl, fr = before[-F:], behind[:F]
            s = np.concatenate([fl, t, fr, mh.ACGT[rng.integers(0, 4, 2)]])   # (two more: what a deletion pulls in)
            starts = [F - d for d in overhangs(L, k)] + [F + T - L + d for d in overhangs(L, k)]
            if T < L:
                starts += [F - ((L - T) * j) // 5 for j in range(6)]
            for a in starts:
                i = len(r1)
                a2 = (a, a - 30, a + 50, F + T + 10 - L)[i % 4]
                mates = []
                for st, fwd in ((a, True), (a2, False)):
                    assert 0 <= st and st + L + 1 <= s.size
                    w = s[st:st + L].copy()
                    edited = False
                    if nread % 7 == 3:
                        w[L // 2] = mh.ACGT[(np.searchsorted(mh.ACGT, w[L // 2]) + 1 + rng.integers(0, 3)) % 4]
                        edited = True
                    if nread % 11 == 5:
                        w = np.delete(s[st:st + L + 1], L // 2)
                        edited = True
                    nread += 1
                    if not fwd:
                        w = mh.COMP[w[::-1]]
                    p = st - F
                    inside = max(0, min(p + L, T) - max(p, 0))
                    runs_on = any((p < 0 and o > 0 and u[o - 1] == s[F - 1]) or (p + L > T and o + T < u.size and u[o + T] == s[F + T]) for u, o in inside_of)
                    mates.append((w.tobytes(), (ti, p, fwd, edited, random_flanks, inside, runs_on)))
                if i % 8 >= 4:                                          # (every kind of mate 2 both ways round)
                    mates.reverse()
                r1.append(mates[0][0]); r2.append(mates[1][0]); truth.append((mates[0][1], mates[1][1]))
    return r1, r2, truth


def reads_for(k, L, seed=READS_SEED):
    """reads() over txome(k), packed: -> {"r1", "r2", "truth", "q1", "o1", "q2", "o2", "n", "lens" (of the transcripts)}"""
    def make():
        from util import pack
        names, seqs = txome(k)
        r1, r2, truth = reads(seqs, L, k, seed)
        q1, o1 = pack(r1); q2, o2 = pack(r2)
        assert set(np.diff(o1)) == {L} and set(np.diff(o2)) == {L}
        return {"r1": r1, "r2": r2, "truth": truth, "q1": q1, "o1": o1, "q2": q2, "o2": o2, "n": len(r1), "lens": np.array([s.size for s in seqs], dtype=np.int64)}
    return mh.once(("ends_reads_for", k, L, seed), make)


# ---- the checks

def reach(res, txp_lens, L):
    """(negative, past_end, on_short) of a result's hits: with pos < 0, with pos + L beyond the transcript's last character, on a
    transcript shorter than the read.  Asked of the ORACLE's result: whether the data reaches the edges, not whether the code is right."""
    h = res.hits
    tl = np.asarray(txp_lens, dtype=np.int64)[h["tid"].astype(np.int64)]
    pos = h["pos"].astype(np.int64)
    return int((pos < 0).sum()), int((pos + L > tl).sum()), int((tl < L).sum())


def assert_reach(res, txp_lens, L, variant, what):
    """the minimums every test that maps this data asserts, on the oracle's result `res` under option set `variant`; -> reach()"""
    got = reach(res, txp_lens, L)
    if variant.startswith("mimic"):
        # alignment policies 1 and 2 drop an alignment that hangs over an end (qm_sel.inl, sel_side_score: `dropped`)
        assert got[0] == 0 and got[1] == 0 and len(res.hits) >= 1, (what, got, len(res.hits))
    elif variant.startswith("selAln"):
        assert got[0] >= REACH_SEL_NEGATIVE, (what, got)
    elif variant == "default":
        assert all(g >= m for g, m in zip(got, REACH_DEFAULT)), (what, got)
    return got


def truth_check(hit_offsets, hits, truth, single=None):
    """Every mate that carries no edit, was cut between random flanks and has 2 k characters or more inside its transcript (covered()
    below sets every other entry of truth to None) has its own transcript among its unit's hits, on the strand it was cut from, at the
    position it was cut from.  Nothing here goes through the oracle or the suffix array.  Paired units: mate 1 is `pos` / `fwd` of a record
    that is paired or a left orphan, mate 2 is `mate_pos` / `mate_is_fwd` of a paired record or `pos` / `fwd` of a right orphan.
    single: the truth entries of single-end units instead.  -> (mates checked, of them with a negative true position)

    The position of a left overhang: an orphan's and a single-end read's record holds the negative start itself (position of the first
    k-mer found minus its place in the read); a PAIRED record holds max(start, 0) for either mate -- the reference's merge writes
    startRead1 = max(leftIt->pos, 0) and startRead2 = max(rightIt->pos, 0) into the joint hit (RapMapUtils.hpp:1212-1227), which is
    what the first run of this check on the oracle's hits showed: about 600 of 1 550 covered mates "missing", every one of them at 0 in
    a paired record.
    What the collector misses (SACollector.hpp:550-673): it looks every k-mer of the read up until one is found (a miss moves on by one
    character), so 2 k characters inside hold a k-mer of the transcript whatever the flank; but it then takes the MAXIMAL match from there
    and keeps the suffix-array interval of that whole match.  Where t also lies inside a longer transcript u (the sub_* transcripts) and
    the flank's first character happens to be u's next one, the match runs on by that character and its interval no longer holds t's
    suffix, which has a `$` there: 25 mates of sub_first80 at k = 31, all cut between the same flanks.  reads() marks such a mate `runs on`
    from the sequences alone, and covered() leaves it out, together with the other mate of its pair (3 more at k = 31: that mate's hit
    on t finds no partner there, and a unit with paired records reports no orphans).  Every other covered mate survives the merge,
    because whatever transcript the other mate hits through characters of t, it hits t too."""
    hits = np.asarray(hits)
    missing, checked, negative = [], 0, 0
    units = [(i, (e,)) for i, e in enumerate(single)] if single is not None else list(enumerate(truth))
    for i, mates in units:
        h = hits[hit_offsets[i]:hit_offsets[i + 1]]
        for m, e in enumerate(mates):
            if e is None:
                continue
            ti, p, fwd, edited, random_flanks, inside, runs_on = e
            assert not edited and random_flanks and not runs_on
            own = h[h["tid"] == ti]
            if single is not None:
                ok = ((own["pos"] == p) & (own["fwd"] == fwd)).any()
            elif m == 0:
                ok = ((own["fwd"] == fwd) & (((own["pos"] == max(p, 0)) & (own["mate_status"] == 3)) | ((own["pos"] == p) & (own["mate_status"] == 1)))).any()
            else:
                ok = (((own["mate_pos"] == max(p, 0)) & (own["mate_is_fwd"] == fwd) & (own["mate_status"] == 3)) |
                      ((own["pos"] == p) & (own["fwd"] == fwd) & (own["mate_status"] == 2))).any()
            checked += 1
            negative += p < 0
            if not ok:
                missing.append((i, m, e))
    assert not missing, "%d of %d mates lack their own transcript, strand and position among their unit's hits, first (unit, mate, truth): %r" % (len(missing), checked, missing[0])
    assert negative >= 200, "only %d of the %d mates checked have a negative true position" % (negative, checked)
    return checked, negative


def covered(truth, k, paired=True):
    """truth with every mate that truth_check does not cover set to None: edited, neighbour flanks, fewer than 2 k characters inside, runs
    on -- or, in a pair, the OTHER mate runs on: that mate then pairs up on the longer transcripts alone, and a unit that has paired
    records reports no orphans, so this mate's hit on t goes unreported"""
    keep = lambda e: e if (not e[3] and e[4] and e[5] >= 2 * k and not e[6]) else None
    return [(keep(a), keep(b)) if not (paired and (a[6] or b[6])) else (None, None) for a, b in truth]


def covered_single(truth, k):
    """covered() for the units of odd_single(reads1, reads2): one entry (or None) per single-end read"""
    one = [a for a, b in truth[:-1]] + [truth[1][1]]
    if len(one) % 2 == 0:
        one = one[:-1]
    return [a for a, b in covered([(e, e) for e in one], k, paired=False)]


# ---- the option sets (mapping_harness.OPTION_SETS)

OPTION_SETS = ("default", "noSensitive", "fuzzy", "noDovetail", "noOrphans", "noStrictCheck", "z0.9", "selAln", "selAln_hardFilter", "selAln_fullband",
               "mimicBT2", "mimicStrictBT2")
FEW = ("default", "fuzzy", "selAln", "mimicBT2")


def report(what, n, res, got_reach):
    """the line every test prints per configuration: the record of what ran (profiles/txp_ends/results)"""
    print("%s: %d units, %d hits, pos<0 %d, past the end %d, on a transcript shorter than the read %d" % ((what, n, len(res.hits)) + tuple(got_reach)))


def after_ref(res, rd, L, variant, what):
    """mapping_harness.ref's hook: every oracle result of this data has its reach asserted and reported when it is computed"""
    report("oracle, " + what, len(res.hit_offsets) - 1, res, assert_reach(res, rd["lens"], L, variant, what))
