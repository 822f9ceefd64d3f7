"""Families of T transcripts around a shared core: data of test_txp_fanout.py (the lane emulation of the device source) and
test_txp_fanout_gpu.py (the HIP path).  A read cut from a core lies in all T members of its family, so its suffix-array interval holds
T suffixes, one per transcript: the hits-to-mappings pass of the lean and pair kernels (lean_h2m, qm_lean.inl; qm_duo.inl) then works on
n = T entries -- or on 2 T, from two intervals, when the read carries one substitution.  T takes the sizes at which that pass changes
its way: 1, 2, either side of 8 (one tile of the wavefront), of 16 and of 32 (where the tiles end, and where two intervals of T
suffixes no longer fit the 64-entry stash and the read is left to the general kernel).

Every T comes twice: a plain family (all members hold the same core), and a diverging one, where member j holds a substitution at
core position DIVERGE[j % 3] (none for j % 3 == 0): the maximal match of a read that crosses such a position goes on in the members that
agree with it only, so its interval is narrower than the one in front of the read's own substitution, and the transcripts that are missing
from it are dropped.

The flanks are random and of random lengths (the position of the core differs from member to member); two members never hold the same
sequence, so the indexer keeps them all.  The seeds: default_rng(TXOME_SEED * 1000 + k) for the transcripts; the reads are cut at fixed
places.  The reference is the oracle.  No test functions here."""
import numpy as np

import mapping_harness as mh

TXOME_SEED = 71
SIZES = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33)
CORE = 150
DIVERGE = (None, 75, 120)
WINDOWS = (0, 50)                                   # where mate 1 starts in the core; mate 2: the reverse complement of core[50:150]
VARIANTS = ("default", "m3", "maxInterval50")


def rc(a):
    return mh.COMP[a[::-1]]


def _other(c):
    return mh.ACGT[(np.searchsorted(mh.ACGT, c) + 1) % 4]


def txome(k, seed=TXOME_SEED):
    """-> {"names", "seqs", "families": [(T, diverging?, [the members' transcripts], [where the core starts in each])]}"""
    def make():
        rng = np.random.default_rng(seed * 1000 + k)
        rand = lambda n: mh.ACGT[rng.integers(0, 4, n)]
        names, seqs, fams = [], [], []
        for T in SIZES:
            for div in (False, True):
                core = rand(CORE)
                ids, starts = [], []
                for j in range(T):
                    c = core.copy()
                    at = DIVERGE[j % 3] if div else None
                    if at is not None:
                        c[at] = _other(c[at])
                    l, r = rand(int(rng.integers(40, 121))), rand(int(rng.integers(40, 121)))
                    names.append("fan_T%d_%s_%d" % (T, "div" if div else "plain", j)); seqs.append(np.concatenate([l, c, r]))
                    ids.append(len(seqs) - 1); starts.append(l.size)
                fams.append((T, div, ids, starts))
        assert len({s.tobytes() for s in seqs}) == len(seqs), "two equal transcripts: the indexer would drop one"
        return {"names": names, "seqs": seqs, "families": fams}
    return mh.once(("fanout_txome", k, seed), make)


def index_for(tmp_root, k, image, seed=TXOME_SEED):
    def make():
        tx = txome(k, seed)
        return mh.index_of(tmp_root, "fanout", k, image, tx["names"], tx["seqs"])
    return mh.once(("fanout_index", k, image, seed), make)


def reads(tx, L):
    """-> (reads1, reads2, truth).  From member 0 of every family -- and from member 1 of a diverging one, which holds the substitution at
    core position 75 -- for every window of WINDOWS three pairs: as cut; one substitution at position 40 of mate 1 (two intervals); one at
    position 60 of mate 2.  Pair i: i % 3 == 1 -- the mates swapped; 2 -- both reverse-complemented.
    truth[i] = (T, diverging?, source member, window, which mate carries the substitution or 0)"""
    assert L == 100, L
    r1, r2, truth = [], [], []
    for (T, div, ids, starts) in tx["families"]:
        for src in ((0, 1) if div and T > 1 else (0,)):
            core = tx["seqs"][ids[src]][starts[src]:starts[src] + CORE]
            for a0 in WINDOWS:
                for err in (0, 1, 2):
                    a, b = core[a0:a0 + L].copy(), rc(core[50:50 + L])
                    if err == 1:
                        a[40] = _other(a[40])
                    if err == 2:
                        b[60] = _other(b[60])
                    kind = len(r1) % 3
                    if kind == 1:
                        a, b = b, a
                    if kind == 2:
                        a, b = rc(a), rc(b)
                    r1.append(a.tobytes()); r2.append(b.tobytes()); truth.append((T, div, src, a0, err))
    return r1, r2, truth


def reads_for(k, L):
    def make():
        from util import pack
        tx = txome(k)
        r1, r2, truth = reads(tx, L)
        q1, o1 = pack(r1); q2, o2 = pack(r2)
        return {"r1": r1, "r2": r2, "truth": truth, "q1": q1, "o1": o1, "q2": q2, "o2": o2, "n": len(r1), "lens": np.array([s.size for s in tx["seqs"]], dtype=np.int64)}
    return mh.once(("fanout_reads_for", k, L), make)


def reach(res):
    """asked of the ORACLE's result (mapped with want_ints=True): -> (the widths of the intervals of reads with ONE interval on a strand, the
    (wider, narrower) width pairs of reads with TWO intervals of different widths on a strand)"""
    one, two = set(), set()
    w = (res.ints[:, 1] - res.ints[:, 0]).astype(np.int64)
    lst = res.ints[:, 5]
    for u in range(len(res.ints_offsets) - 1):
        a, b = int(res.ints_offsets[u]), int(res.ints_offsets[u + 1])
        for l in range(4):
            ws = w[a:b][lst[a:b] == l]
            if ws.size == 1:
                one.add(int(ws[0]))
            elif ws.size == 2 and ws[0] != ws[1]:
                two.add((int(ws.max()), int(ws.min())))
    return one, two
