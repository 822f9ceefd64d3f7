"""Reads and cases that more than one test module uses and no family's case module holds: the `$` reads and the -s cases of
test_emu_parity.py and test_gpu_parity.py, the ksw2 inputs of test_ksw_variants.py and test_oracle_ref.py.  No test functions here."""
import os

import numpy as np

from conftest import GOLD


def dollar_reads(sd):
    """reads with a '$' (the text's separator) spliced in, incl. right after the seed k-mer and at the last base"""
    r1 = [bytearray(r) for r in sd["reads1"][:400]]
    r2 = [bytearray(r) for r in sd["reads2"][:400]]
    for i, r in enumerate(r1):
        if len(r) > 40:
            r[(31, 40, len(r) - 1, 5)[i % 4]] = ord("$")
    for i, r in enumerate(r2[::3]):
        if len(r) > 60:
            r[60] = ord("$")
    return [bytes(r) for r in r1], [bytes(r) for r in r2]


SEL_VARIANTS = [
    ("reads", dict(selAln=1), dict(sel_aln=1)),
    ("indel", dict(selAln=1), dict(sel_aln=1)),
    ("reads", dict(selAln=1, hardFilter=1), dict(sel_aln=1, hard_filter=1)),
    ("indel", dict(selAln=1, maxMMPExtension=3, minScoreFraction=0.9), dict(sel_aln=1, max_mmp_extension=3, min_score_fraction=0.9)),
    ("reads", dict(selAln=1, noOrphans=1, noDovetail=1, consensusSlack=0.35, maxNumHits=1000, alnPolicy=1),
     dict(sel_aln=1, no_orphans=1, no_dovetail=1, consensus_slack=0.35, max_num_hits=1000, aln_policy=1)),          # --mimicBT2
    ("indel", dict(selAln=1, consensusSlack=0.0, gapOpen=6, gapExtend=3, mismatchPenalty=-6, matchScore=3, dpBandwidth=5),
     dict(sel_aln=1, consensus_slack=0.0, gap_open=6, gap_extend=3, mismatch_penalty=-6, match_score=3, dp_bandwidth=5)),
    # without --strictCheck the other strand's turn depends on the two spot-check counts (hb >= ha): the lean collector's runs of
    # capped MMPs book several hits' counts at once
    ("reads", dict(selAln=1, strictCheck=0), dict(sel_aln=1, strict_check=0)),
    ("indel", dict(selAln=1, strictCheck=0, maxMMPExtension=3), dict(sel_aln=1, strict_check=0, max_mmp_extension=3)),
]


def sel_reads(synth_small, which):
    import samfmt as sam
    if which == "reads":
        return synth_small["reads1"], synth_small["reads2"]
    nx = os.path.join(GOLD, "synth_small", "next")
    return sam.read_fastq(os.path.join(nx, "reads_indel_1.fastq.gz"))[1], sam.read_fastq(os.path.join(nx, "reads_indel_2.fastq.gz"))[1]


def _edited_pairs(txps, n, seed):
    """pairs of 100-bp reads (mate 2 from the other strand, 150 bases downstream) with the edits that decide between the gapless
    path and a path with one gap: two substitutions anywhere, or a one- / two-base deletion or a one-base insertion a few
    characters from either end of the read (behind it the diagonal has a handful of mismatches, often exactly two)"""
    rng = np.random.default_rng(seed)
    B = np.frombuffer(b"ACGT", dtype=np.uint8)
    comp = np.zeros(256, np.uint8); comp[list(b"ACGT")] = list(b"TGCA")
    long_enough = [t for t in txps if len(t) >= 400]

    def edit(frag):                                         # frag: 104 characters of transcript, the read is (about) its first 100
        kind = int(rng.integers(0, 6))
        r = frag.copy()
        if kind == 0:
            for p in rng.choice(100, 2, replace=False): r[p] = B[(np.searchsorted(B, r[p]) + 1 + rng.integers(0, 3)) % 4]
            return r[:100]
        near = int(rng.integers(1, 7))
        p = near if rng.random() < 0.5 else 100 - near
        if kind in (1, 2): return np.concatenate([r[:p], r[p + 1:]])[:100]                   # one base missing from the read
        if kind == 3: return np.concatenate([r[:p], r[p + 2:]])[:100]                        # two
        if kind == 4: return np.concatenate([r[:p], B[rng.integers(0, 4, 1)], r[p:]])[:100]  # one extra
        for p in rng.choice(100, 3, replace=False): r[p] = B[(np.searchsorted(B, r[p]) + 1) % 4]
        return r[:100]
    r1, r2 = [], []
    for i in range(n):
        t = long_enough[int(rng.integers(0, len(long_enough)))]
        p = int(rng.integers(0, len(t) - 360))
        a = edit(t[p:p + 104]); b = edit(t[p + 150:p + 254])
        b = comp[b[::-1]]
        if i % 2: a, b = b, a
        r1.append(a.tobytes()); r2.append(b.tobytes())
    return r1, r2


# the schemes of test_selective_alignment_answers_known_without_ksw2 (emulation and device), as oracle options
KNOWN_ANSWER_SCHEMES = [dict(), dict(gapOpen=4, gapExtend=2), dict(matchScore=1, mismatchPenalty=-1, gapOpen=1, gapExtend=1),
                        dict(dpBandwidth=5), dict(matchScore=2, mismatchPenalty=-4, gapOpen=6, gapExtend=1, dpBandwidth=-1)]
KNOWN_ANSWER_OPTS = {"gapOpen": "gap_open", "gapExtend": "gap_extend", "matchScore": "match_score", "mismatchPenalty": "mismatch_penalty", "dpBandwidth": "dp_bandwidth"}


def ksw_mutate(rng, q, tlen, sub=0.05, indel=0.02, nfrac=0.01):
    """a target of tlen codes: the query (repeated as needed) with substitutions, insertions, deletions and N's"""
    out = []
    i = 0
    while len(out) < tlen:
        r = rng.random()
        if r < indel:            # insertion in the target
            out.append(rng.integers(0, 4))
        elif r < 2 * indel:      # deletion
            i += 1
        else:
            c = q[i % len(q)]
            if rng.random() < sub:
                c = rng.integers(0, 4)
            if rng.random() < nfrac:
                c = 4
            out.append(c); i += 1
    return np.array(out[:tlen], dtype=np.uint8)


def ksw_cases(seed, n):
    """n (query, target) pairs of codes 0 .. 4 for the ksw2 extension kernel: random lengths, the target a mutated copy or random"""
    rng = np.random.default_rng(seed)
    for it in range(n):
        qlen = int(rng.integers(1, 141))
        tlen = int(rng.integers(1, 161)) if it % 3 else min(160, qlen + 20)
        q = rng.integers(0, 4, qlen).astype(np.uint8)
        if rng.random() < 0.1:
            q[rng.integers(0, qlen)] = 4
        t = ksw_mutate(rng, q, tlen) if rng.random() < 0.85 else rng.integers(0, 5, tlen).astype(np.uint8)
        yield q, t
