"""Inputs and restatements of the tests of the -s question scorer and the strip alignments by themselves (test_sel_side.py: lane emulation,
test_sel_side_gpu.py: device): sel_side_score and sel_tasks_strip of rapmap_amd/csrc/qm_sel.inl.  No test functions here.

A question is what getAlnScore (SelectiveAlignmentUtils.hpp:260-373) is asked: a read as it is stored and its orientation, a transcript, a
position, a chain status (UNGAPPED or REGULAR) and whether the unit is multi-mapping; the alignment policy and the scoring scheme
(match, mismatch, gap open, gap extend, band) are arguments of a launch, so a Batch of questions is scored under one policy and scheme.

The restatements: _known_answer_rule (the two rules of sel_side_score), _strip_dp (sel_tasks_strip) -- test_ksw_variants.py holds both against
the oracle's qo_ksw_extz2 -- and classify(), the geometry of getAlnScore plus which of the two rules or the strip answers a question.
The reference of every score is qo_ksw_extz2 on the nt4 codes of the read slice in alignment orientation and of target[:tlen1]; for an UNGAPPED
chain the plain per-character count of getAlnScore's ungappedAln.  Everything is compared as exact integers."""
import collections
import ctypes as C
import functools

import numpy as np

from oracle import oracle

UNGAPPED, REGULAR = 1, 4                                          # rapmap::utils::ChainStatus
LOWEST = -(1 << 31)
CLASSES = ("dropped", "off_end", "ungapped", "known", "strip", "ksw2")
MAX_READ_LEN = 512                                                # QM_MAX_READ_LEN: longer reads never go to the strip kernel

# the scheme lists of test_ksw_variants.py's three rule tests, and band 0 (no rule applies: every REGULAR question is ksw2's)
SCHEMES = [(2, -4, 4, 2, 15), (2, -4, 4, 2, 1), (2, -4, 4, 2, 5), (1, -1, 1, 1, 15), (2, -6, 5, 3, 33), (4, -4, 6, 2, 20), (2, -4, 4, 2, 98),
           (2, -4, 4, 2, -1), (3, -2, 2, 1, 15), (1, 0, 25, 25, 15), (2, -4, 5, 3, 15), (2, -4, 4, 2, 8), (2, -4, 5, 3, 9), (1, -3, 2, 1, 15),
           (2, -4, 6, 1, 15), (2, -4, 4, 2, 0)]
LENGTHS = list(range(1, 10)) + [15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 250, 512]

Question = collections.namedtuple("Question", "read fwd tx pos cs multi")     # read, tx: uint8 arrays of characters


# ---------------------------------------------------------------------------------------------------------------- restatements
def _known_answer_rule(q, t, a, b, q_, e_, w):
    """returns score or None (ask ksw2)"""
    qlen, tlen = len(q), len(t)
    aa, bb = abs(a), -abs(b)
    M = aa - bb; qe = q_ + e_
    if not (w != 0 and tlen >= qlen and qlen > 0 and aa >= 1 and q_ >= 0 and e_ >= 1 and aa - bb + qe <= 96): return None
    sc = np.where((q < 4) & (t[:qlen] < 4), np.where(q == t[:qlen], aa, bb), 0)
    smax = int(np.where(q < 4, aa, 0).sum()); U = int(sc.sum()); loss = smax - U
    if loss <= qe: return U
    # extension
    if M > qe or loss != 2 * M: return None
    Ld = 0
    while q_ + (Ld + 1) * e_ < 2 * M: Ld += 1
    Li = 0
    while q_ + (Li + 1) * (e_ + aa) < 2 * M: Li += 1
    if Ld > 3 or Li > 2: return None
    if not (w < 0 or w >= 8): return None
    if tlen < qlen + Ld + 1: return None
    if qlen < Ld or qlen <= Li: return None               # (a query of one or two characters: see qm_sel.inl, and DESIGN.md on what these tests found)
    if (q >= 4).any() or (t[:qlen + Ld] >= 4).any(): return None
    mm = np.nonzero(q != t[:qlen])[0]
    assert len(mm) == 2
    m1 = int(mm[0])
    best = 2 * M
    for L in range(1, Ld + 1):
        d = np.nonzero(q != t[L:L + qlen])[0]
        hm = int(d[-1]) if len(d) else -1
        if hm <= m1 - 1: best = min(best, q_ + L * e_)
    for L in range(1, Li + 1):
        idx = np.arange(L, qlen)
        d = idx[q[L:] != t[:qlen - L]]
        hm = int(d[-1]) if len(d) else L - 1
        if hm <= m1 + L - 1: best = min(best, q_ + L * (e_ + aa))
    return smax - best


NEG = -(1 << 28)

def _strip_dp(q, t, a, b, go, ge, half=7):
    """extension alignment from (0,0), affine gaps go + L*ge, score-only, max(mqe, mte); diagonals -half .. half+1"""
    qlen, tlen = len(q), len(t)
    aa, bb = abs(a), -abs(b)
    W = 2 * half + 2
    Hp = [NEG] * W; Fp = [NEG] * W
    for c in range(W):
        j = c - (half + 1)
        if j == -1: Hp[c] = 0
        elif 0 <= j < tlen: Hp[c] = -(go + ge * (j + 1))
    mqe = NEG; mte = NEG
    for i in range(qlen):
        Ht = [NEG] * W; F = [NEG] * W
        for c in range(W):
            j = i + c - half
            if j == -1:
                Ht[c] = -(go + ge * (i + 1)); continue
            if j < 0 or j >= tlen: continue
            s = (aa if q[i] == t[j] else bb) if (q[i] < 4 and t[j] < 4) else 0
            M = Hp[c] + s if Hp[c] > NEG else NEG
            f = NEG
            if c + 1 < W:
                if Hp[c + 1] > NEG: f = Hp[c + 1] - go - ge
                if Fp[c + 1] > NEG: f = max(f, Fp[c + 1] - ge)
            F[c] = f
            Ht[c] = max(M, f)
        H = [NEG] * W
        run = NEG
        for c in range(W):
            j = i + c - half
            E = run - go - ge * c if run > NEG else NEG
            if j == -1: H[c] = Ht[c]
            elif 0 <= j < tlen: H[c] = max(Ht[c], E)
            if Ht[c] > NEG: run = max(run, Ht[c] + ge * c)
            if 0 <= j < tlen:
                if i == qlen - 1: mqe = max(mqe, H[c])
                if j == tlen - 1: mte = max(mte, H[c])
        Hp, Fp = H, F
    return max(mqe, mte)


NT4 = np.full(256, 4, dtype=np.uint8)                             # seq_nt4_table_loc (KSW2Aligner.cpp:61-72)
for _i, _c in enumerate(b"ACGT"):
    NT4[_c] = _i; NT4[_c | 0x20] = _i
NT4[:4] = np.arange(4)
RC = np.full(128, ord("N"), dtype=np.uint8)                       # rc_table of reverseRead (src/RapMapUtils.cpp:63-72)
for _c, _d in zip(b"ACGTU", b"TGCAA"):
    RC[_c] = _d; RC[_c | 0x20] = _d
_LETTER = np.zeros(256, dtype=bool)
_LETTER[list(b"ACGTacgt")] = True


def aligned_read(read, fwd):
    """the read as the alignment sees it: as it is, or reverseRead() of it"""
    return read if fwd else RC[read[::-1]]


def limits(scheme):
    """which shortcuts the scheme admits at all: (rule 1, rule 2, Ld, Li, strip) -- sel_side_score's own limits"""
    a, b, gq, ge, w = scheme
    aa, bb = abs(a), -abs(b)
    M = aa - bb
    diag = w != 0 and aa >= 1 and gq >= 0 and ge >= 1 and M + gq + ge <= 96
    Ld = 0
    while Ld < 4 and gq + (Ld + 1) * ge < 2 * M: Ld += 1
    Li = 0
    while Li < 3 and gq + (Li + 1) * (ge + aa) < 2 * M: Li += 1
    rule2 = diag and M <= gq + ge and Ld <= 3 and Li <= 2 and (w < 0 or w >= 8)
    return diag, rule2, Ld, Li, diag and (w < 0 or w >= 9)


Geometry = collections.namedtuple("Geometry", "cls roff rlen pos tlen1 key_len ungapped")


def geometry(qn, policy):
    """getAlnScore up to the alignment: invalidStart / invalidEnd, the 20-character buffer, useBuf, keyLen (SelectiveAlignmentUtils.hpp:289-324);
    cls: dropped / off_end / None (scored)"""
    read_len, tlen, pos = len(qn.read), len(qn.tx), qn.pos
    roff, rlen = 0, read_len
    invalid_start, invalid_end = pos < 0, pos + rlen >= tlen
    if invalid_start:
        roff, rlen, pos = -pos, rlen + pos, 0
    if (invalid_start or invalid_end) and policy in (1, 2):
        return Geometry("dropped", roff, rlen, pos, None, None, False)
    if not pos < tlen:
        return Geometry("off_end", roff, rlen, pos, None, None, False)
    ungapped = (not invalid_start) and qn.cs == UNGAPPED
    buf = 0 if ungapped else 20
    lnobuf, lbuf = tlen - pos, rlen + buf
    use_buf = lbuf < lnobuf
    tlen1 = min(lbuf, lnobuf)
    return Geometry(None, roff, rlen, pos, tlen1, tlen1 - buf if use_buf else tlen1, ungapped)


def codes(qn, g):
    """nt4 codes of the read slice in alignment orientation and of target[:tlen1]"""
    rs = aligned_read(qn.read, qn.fwd)[g.roff:g.roff + g.rlen]
    return np.ascontiguousarray(NT4[rs]), np.ascontiguousarray(NT4[qn.tx[g.pos:g.pos + g.tlen1]])


def classify(qn, policy, scheme):
    """-> (class, score or None, roff, rlen, tlen1): who answers the question -- nobody (dropped under the Bowtie-2 policies, off_end: the position
    lies behind the transcript), the ungapped count, one of the two rules (known), the strip kernel or ksw2 -- and, where a restatement gives it,
    the score"""
    a, b, gq, ge, w = scheme
    g = geometry(qn, policy)
    if g.cls:
        return g.cls, None, g.roff, g.rlen, None
    rs = aligned_read(qn.read, qn.fwd)[g.roff:g.roff + g.rlen]
    tw = qn.tx[g.pos:g.pos + g.tlen1]
    if g.ungapped:                                                 # ungappedAln: a character equals itself and 'N' equals everything
        n = min(g.rlen, g.tlen1)
        eq = int(((rs[:n] == tw[:n]) | (rs[:n] == ord("N")) | (tw[:n] == ord("N"))).sum())
        return "ungapped", eq * a + (n - eq) * b, g.roff, g.rlen, g.tlen1
    q, t = NT4[rs], NT4[tw]
    aa, bb = abs(a), -abs(b)
    diag, rule2, Ld, Li, strip = limits(scheme)
    r = _known_answer_rule(q, t, a, b, gq, ge, w)
    loss = None
    if diag and g.tlen1 >= g.rlen and g.rlen > 0:
        loss = int(np.where(q < 4, aa, 0).sum()) - int(np.where((q < 4) & (t[:g.rlen] < 4), np.where(q == t[:g.rlen], aa, bb), 0).sum())
    # a byte below 4 is its own nt4 code; the word-at-a-time scorer answers such a window by rule 1 only (and leaves the rest to the
    # strip or to ksw2, which is always right)
    if r is not None and loss > gq + ge and not (_LETTER[rs].all() and _LETTER[tw[:g.rlen + Ld]].all()):
        r = None
    if r is not None:
        return "known", r, g.roff, g.rlen, g.tlen1
    if strip and loss is not None and loss <= gq + 7 * ge and len(qn.read) <= MAX_READ_LEN:
        return "strip", None, g.roff, g.rlen, g.tlen1
    return "ksw2", None, g.roff, g.rlen, g.tlen1


def ref_score(qq, tt, scheme):
    """the oracle's ksw_extz2 on nt4 codes"""
    a, b, q_, e_, w = scheme
    ol = oracle._lib()
    ol.qo_ksw_extz2.restype = C.c_int
    return ol.qo_ksw_extz2(len(qq), qq.ctypes.data_as(C.c_void_p), len(tt), tt.ctypes.data_as(C.c_void_p), a, b, q_, e_, w)


def winning_diagonals(q, t, scheme):
    """for a question of exactly two mismatches that rule 2 answers: the diagonals (+L: L target characters skipped, -L: L query characters)
    whose one-gap-run path is clean behind the first mismatch and costs what the cheapest of them costs, when that is less than the gapless
    path's 2M -- [] when the gapless path stands"""
    a, b, gq, ge, w = scheme
    aa, bb = abs(a), -abs(b)
    M = aa - bb
    _, rule2, Ld, Li, _ = limits(scheme)
    qlen = len(q)
    mm = np.nonzero(q != t[:qlen])[0]
    if not rule2 or len(mm) != 2 or len(t) < qlen + Ld + 1 or qlen < Ld or qlen <= Li or (q >= 4).any() or (t[:qlen + Ld] >= 4).any():
        return []
    m1 = int(mm[0])
    cost = {}
    for L in range(1, Ld + 1):
        d = np.nonzero(q != t[L:L + qlen])[0]
        if (int(d[-1]) if len(d) else -1) < m1: cost[L] = gq + L * ge
    for L in range(1, Li + 1):
        d = np.arange(L, qlen)[q[L:] != t[:qlen - L]]
        if (int(d[-1]) if len(d) else L - 1) < m1 + L: cost[-L] = gq + L * (ge + aa)
    best = min(cost.values(), default=2 * M)
    return sorted(d for d, c in cost.items() if c == best) if best < 2 * M else []


# ---------------------------------------------------------------------------------------------------------------- a batch
class Batch:
    """questions as the flat arrays both faces take: the reads back to back in one buffer (an over-read brings a neighbour's characters, not
    zeros), the distinct transcripts back to back in one text"""

    def __init__(self, questions):
        self.questions = questions
        self.roffs = np.concatenate([[0], np.cumsum([len(q.read) for q in questions])]).astype(np.int64)
        self.reads = np.concatenate([q.read for q in questions]).astype(np.uint8)
        tid, txs = {}, []
        for q in questions:
            if id(q.tx) not in tid:
                tid[id(q.tx)] = len(txs); txs.append(q.tx)
        self.txp_len = np.array([len(t) for t in txs], dtype=np.int32)
        self.txp_off = np.concatenate([[0], np.cumsum(self.txp_len)[:-1]]).astype(np.uint32)
        self.text = np.concatenate(txs).astype(np.uint8)
        self.qd = np.array([(tid[id(q.tx)], q.pos, 1 if q.fwd else 0, q.cs, 1 if q.multi else 0) for q in questions], dtype=np.int32)

    def __len__(self):
        return len(self.questions)


# ---------------------------------------------------------------------------------------------------------------- questions
B4 = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = np.zeros(256, dtype=np.uint8)
for _c, _d in zip(b"ACGTNacgtn", b"TGCANtgcan"):
    _COMP[_c] = _d
for _c in range(4):
    _COMP[_c] = _c                                               # (reverseRead turns a byte below 4 into 'N': such reads are stored forward)


def _other(rng, c):
    """another letter than c (an upper-case A C G T)"""
    return B4[(int(np.searchsorted(B4, c)) + 1 + int(rng.integers(0, 3))) % 4]


def _stored(rs, fwd):
    """the read whose alignment orientation is rs (up to case)"""
    return np.ascontiguousarray(rs if fwd else _COMP[rs[::-1]])


def _question(rng, rs, tx, pos, fwd=None, cs=None, multi=None, lead=0):
    """rs: the read slice as the alignment is to see it; lead > 0: that many further characters in front of it, hanging over the transcript's
    start (pos is then 0 and the question's position -lead)"""
    fwd = bool(rng.integers(0, 2)) if fwd is None else fwd
    cs = (UNGAPPED if rng.random() < 0.1 else REGULAR) if cs is None else cs
    multi = bool(rng.random() < 0.4) if multi is None else multi
    if lead:
        assert pos == 0
        rs = np.concatenate([B4[rng.integers(0, 4, lead)], rs]); pos = -lead
    return Question(_stored(rs, fwd), fwd, tx, pos, cs, multi)


def _sub(rng, rs, places):
    rs = rs.copy()
    for p in places:
        rs[p] = _other(rng, rs[p])
    return rs


def _edge_places(rlen):
    return sorted({p for p in (0, 7, 8, 15, 16, rlen - 1, rlen - 2) if 0 <= p < rlen})


def substitutions(rng, out):
    """zero to three substitutions on and beside the word boundaries, every length, both orientations; interior positions, and the same read
    hanging over the transcript's start by a few characters"""
    for rlen in LENGTHS:
        tx = B4[rng.integers(0, 4, rlen + 90)]
        places = _edge_places(rlen)
        sets = [()] + [(p,) for p in places] + [(p, r) for i, p in enumerate(places) for r in places[i + 1:]]
        sets += [tuple(rng.choice(places, 3, replace=False)) for _ in range(6) if len(places) >= 3]
        sets += [tuple(rng.choice(rlen, k, replace=False)) for k in (2, 2, 3, 3) if rlen >= k]
        for fwd in (True, False):
            for s in sets:
                pos = int(rng.integers(0, 40))
                out.append(_question(rng, _sub(rng, tx[pos:pos + rlen], s), tx, pos, fwd=fwd, cs=REGULAR))
        for s in sets[::3]:                                        # roff > 0: the alignment starts inside the read
            head = B4[rng.integers(0, 4, rlen + 40)]
            out.append(_question(rng, _sub(rng, head[:rlen], s), head, 0, lead=int(rng.choice([1, 3, 7, 8, 9])), cs=REGULAR))
        for s in sets[::4]:
            pos = int(rng.integers(0, 40))
            out.append(_question(rng, _sub(rng, tx[pos:pos + rlen], s), tx, pos, cs=UNGAPPED))


def many_differences(rng, out, n):
    """four to twelve substitutions, and reads that have nothing to do with the target: what ksw2 is left with"""
    for i in range(n):
        rlen = int(rng.choice([r for r in LENGTHS if r >= 16]))
        tx = B4[rng.integers(0, 4, rlen + 60)]
        pos = int(rng.integers(0, 30))
        k = int(rng.integers(4, 13))
        rs = B4[rng.integers(0, 4, rlen)] if i % 4 == 0 else _sub(rng, tx[pos:pos + rlen], rng.choice(rlen, k, replace=False))
        out.append(_question(rng, rs, tx, pos, cs=REGULAR))


def position_edges(rng, out, scheme):
    """where the geometry changes: a transcript that ends at, inside and right behind the 20-character buffer (tlen1 == rlen + Ld and
    rlen + Ld + 1 among them), reads that reach or pass its end, positions at and behind its end, reads hanging over its start"""
    Ld = limits(scheme)[2]
    for rlen in (1, 3, 8, 9, 17, 33, 100):
        for fwd in (True, False):
            for rest in sorted({0, 1, 2, 3, 4, 5, 8, 19, 20, 21, 22, Ld, Ld + 1}):     # transcript characters behind the read's last one
                for nsub in (0, 2, 3):
                    if nsub > rlen: continue
                    tx = B4[rng.integers(0, 4, 30 + rlen + rest)]
                    rs = _sub(rng, tx[30:30 + rlen], rng.choice(rlen, nsub, replace=False))
                    out.append(_question(rng, rs, tx, 30, fwd=fwd, cs=REGULAR if nsub else None))
            for over in (1, 3, rlen - 1, rlen, rlen + 5):          # the read passes the end by `over` characters / starts at or behind it
                tx = B4[rng.integers(0, 4, 50)]
                rs = np.concatenate([tx[50 - rlen + over:], B4[rng.integers(0, 4, rlen)]])[:rlen]
                out.append(_question(rng, rs, tx, 50 - rlen + over, fwd=fwd))
            for lead in (1, 2, 7, 8, 9, 20):                       # roff > 0
                tx = B4[rng.integers(0, 4, rlen + 25)]
                out.append(_question(rng, _sub(rng, tx[:rlen], rng.choice(rlen, min(rlen, int(rng.integers(0, 3))), replace=False)), tx, 0, fwd=fwd, lead=lead))


def short_and_far(rng, out):
    """reads of one to nine characters that differ from the target everywhere or nearly, the transcript ending 0 .. 21 characters behind them: the
    alignments whose best path runs along the strip's outermost diagonals and ends in the target's last column"""
    for rlen in range(1, 10):
        for rest in range(0, 22):
            tx = B4[rng.integers(0, 4, 12 + rlen + rest)]
            k = rlen if rest % 2 else max(1, rlen - 1)
            rs = _sub(rng, tx[12:12 + rlen], rng.choice(rlen, k, replace=False))
            out.append(_question(rng, rs, tx, 12, cs=REGULAR))


def odd_characters(rng, out, n):
    """N, lower case, bytes below 4 and other letters, in the read and in the target, inside the compared window and right behind it"""
    odd = [ord("N"), ord("n"), 0, 1, 2, 3, ord("R"), ord("U"), ord("u"), ord("-")]
    for i in range(n):
        rlen = int(rng.choice(LENGTHS))
        tx = B4[rng.integers(0, 4, rlen + 70)].copy()
        pos = int(rng.integers(0, 30))
        if i % 5 == 0:
            tx = tx | 0x20                                         # a soft-masked transcript
        rs = (tx[pos:pos + rlen] & 0xdf).copy()
        if i % 7 == 0:
            rs = rs | 0x20
        rs = _sub_any(rng, rs, rng.choice(rlen, min(rlen, int(rng.integers(0, 4))), replace=False))
        fwd = bool(rng.integers(0, 2))
        for _ in range(int(rng.integers(0, 3))):
            c = int(rng.choice(odd))
            rs[int(rng.integers(0, rlen))] = c if fwd or c >= 4 else ord("N")
        for _ in range(int(rng.integers(0, 3))):
            tx[pos + int(rng.choice([rng.integers(0, rlen), rlen + rng.integers(0, 4)]))] = int(rng.choice(odd))
        out.append(_question(rng, rs, tx, pos, fwd=fwd, cs=UNGAPPED if i % 6 == 0 else REGULAR))


def _sub_any(rng, rs, places):
    rs = rs.copy()
    for p in places:
        c = _other(rng, rs[p] & 0xdf)
        rs[p] = c | (rs[p] & 0x20)
    return rs


def loss_grid(rng, out, n):
    """k substitutions and j N's in the target under the read: losses k M + j a on both sides of q + e, 2M and q + 7e"""
    for i in range(n):
        rlen = int(rng.choice([r for r in LENGTHS if r >= 31]))
        tx = B4[rng.integers(0, 4, rlen + 50)].copy()
        pos = int(rng.integers(0, 25))
        k, j = int(rng.integers(0, 6)), int(rng.integers(0, 5))
        places = rng.choice(rlen, k + j, replace=False)
        rs = _sub(rng, tx[pos:pos + rlen], places[:k])
        tx[pos + places[k:]] = ord("N")
        out.append(_question(rng, rs, tx, pos, cs=REGULAR))


def scaled_losses(rng, out, scheme, n_known, n_strip, n_ksw2):
    """k substitutions (and a few N's) with k drawn from the scheme's own bands: a loss of at most q + e (rule 1), of at most q + 7e (the strip),
    and beyond (ksw2) -- whatever M, q and e are, each class gets its questions"""
    a, b, gq, ge, w = scheme
    aa, M = abs(a), abs(a) + abs(b)
    k1, k7 = (gq + ge) // M, (gq + 7 * ge) // M
    for lo, hi, n in ((0, k1, n_known), (k1 + 1, k7, n_strip), (k7 + 1, k7 + 6, n_ksw2)):
        for _ in range(n if hi >= lo else 0):
            k = int(rng.integers(lo, hi + 1))
            fit = [r for r in LENGTHS if r >= max(k + 2, 10)]
            if not fit: continue
            rlen = int(rng.choice(fit[:12]))
            tx = B4[rng.integers(0, 4, rlen + 50)].copy()
            pos = int(rng.integers(0, 25))
            j = int(rng.integers(0, min(2, max(0, (gq + ge - k * M)) // aa) + 1)) if hi == k1 else 0
            places = rng.choice(rlen, k + j, replace=False)
            rs = _sub(rng, tx[pos:pos + rlen], places[:k])
            tx[pos + places[k:]] = ord("N")
            out.append(_question(rng, rs, tx, pos, cs=REGULAR))


def tiny_slices(rng, out):
    """alignments of one to four characters -- short reads, and the last characters of a read that hangs over the transcript's start --, all of
    them different from the target or equal to its next diagonal, an N here and there right behind them: shorter than the gap runs rule 2 weighs"""
    for rlen in (1, 2, 3, 4):
        for i in range(40):
            tx = B4[rng.integers(0, 4, 40)].copy()
            shift = int(rng.integers(0, 4))
            rs = tx[shift:shift + rlen].copy() if i % 2 else _sub(rng, tx[:rlen], range(rlen))
            if i % 4 >= 2:
                tx[rlen + int(rng.integers(0, 3))] = ord("N")
            lead = int(rng.choice([0, 3, 9]))
            txq = tx if lead else np.concatenate([B4[rng.integers(0, 4, 5)], tx])
            out.append(_question(rng, rs, txq, 0 if lead else 5, cs=REGULAR, lead=lead))


def end_indels(rng, out, scheme, per_diagonal):
    """an indel of length L within the last one to seven characters of a read on random text: behind it the main diagonal mismatches almost
    everywhere, and when it does so exactly twice the one-gap path wins (the source of the gap-wins floor); proposals whose main diagonal has
    other than two mismatches are mostly passed over, the gap-wins floor is what counts the rest"""
    _, rule2, Ld, Li, _ = limits(scheme)
    if not rule2:
        Ld, Li = 3, 2                                              # (the scheme answers none of these by rule 2: a few for the other classes)
        per_diagonal = per_diagonal // 8
    lens = [r for r in LENGTHS if 9 <= r <= 129]
    for d in list(range(1, Ld + 1)) + [-L for L in range(1, Li + 1)]:
        kept = 0
        for _ in range(40 * per_diagonal):
            if kept >= per_diagonal: break
            rlen = int(rng.choice(lens)); L = abs(d)
            lead = int(rng.choice([0, 0, 0, 1, 5, 8]))
            tx = B4[rng.integers(0, 4, rlen + 60)]
            pos = 0 if lead else int(rng.integers(0, 30))
            k = rlen - int(rng.integers(1, 8))
            w = tx[pos:pos + rlen + 8]
            rs = np.concatenate([w[:k], w[k + L:]])[:rlen] if d > 0 else np.concatenate([w[:k], B4[rng.integers(0, 4, L)], w[k:]])[:rlen]
            two = int((rs != w[:rlen]).sum()) == 2
            if not two and rng.random() > 0.1: continue
            kept += two
            out.append(_question(rng, rs, tx, pos, cs=REGULAR, lead=lead))


def clean_diagonal_thresholds(rng, out, scheme, reps):
    """two mismatches m1 < m2 on the main diagonal and a neighbouring diagonal that is clean from exactly s on (it mismatches at s - 1), for s one
    before, at and one behind the last start the rule accepts -- m1 for +1 +2 +3, m1 + L for -1 -2"""
    _, rule2, Ld, Li, _ = limits(scheme)
    if not rule2: return
    for d in list(range(1, Ld + 1)) + [-L for L in range(1, Li + 1)]:
        L = abs(d)
        for rep in range(reps):
            for ds in (-1, 0, 1):
                rlen = int(rng.choice([r for r in LENGTHS if r >= 9 and r <= 129]))
                m1 = int(rng.integers(max(2, L + 1), rlen - 2)) if rep % 3 else int(rng.choice([p for p in (7, 8, 15, 16, rlen - 3) if max(2, L + 1) <= p < rlen - 2]))
                m2 = int(rng.integers(m1 + 2, rlen)) if m1 + 2 < rlen else rlen - 1
                s = (m1 if d > 0 else m1 + L) + ds
                if not (L + 1 <= s < rlen) or s - 1 == m2 or (s - 1 == m1 and ds != 1 and d > 0): continue
                n = rlen + 30
                t = B4[rng.integers(0, 4, n)].copy(); rs = np.zeros(rlen, dtype=np.uint8)
                if d > 0:
                    for i in range(s, rlen):                       # clean from s: rs[i] = t[i + L]; off the two mismatches also = t[i]
                        t[i + L] = _other(rng, t[i]) if i in (m1, m2) else t[i]
                        rs[i] = t[i + L]
                    for i in range(s):
                        rs[i] = t[i]
                    if s - 1 not in (m1, m2) and t[s - 1 + L] == t[s - 1]:
                        continue                                   # (diagonal +L would be clean from s - 1 on: another case's)
                else:
                    for i in range(s, rlen):                       # clean from s: rs[i] = t[i - L]
                        t[i] = _other(rng, t[i - L]) if i in (m1, m2) else t[i - L]
                        rs[i] = t[i - L]
                    for i in range(s):
                        rs[i] = t[i]
                    if s - 1 not in (m1, m2) and t[s - 1 - L] == t[s - 1]:
                        continue
                for m in (m1, m2):
                    if m < s:
                        cand = [c for c in B4 if c != t[m] and (m != s - 1 or c != (t[m + L] if d > 0 else t[m - L]))]
                        rs[m] = cand[int(rng.integers(0, len(cand)))]
                # what was built is checked here; what it is worth is classify()'s and the oracle's business
                mm = np.nonzero(rs != t[:rlen])[0]
                dd = np.nonzero(rs != t[L:L + rlen])[0] if d > 0 else np.arange(L, rlen)[rs[L:] != t[:rlen - L]]
                if list(mm) != [m1, m2] or (int(dd[-1]) if len(dd) else -1) != s - 1: continue
                lead = int(rng.choice([0, 0, 3]))
                tx = t if lead else np.concatenate([B4[rng.integers(0, 4, 11)], t])
                out.append(_question(rng, rs, tx, 0 if lead else 11, cs=REGULAR, lead=lead))


def low_complexity(rng, out, n):
    """periodic and low-complexity targets (the neighbouring diagonals do match), substitutions at the ends, true indels: the strip's and rule 2's
    everyday hard cases (the proposals of test_ksw_variants.py's rule tests, as characters)"""
    for it in range(n):
        rlen = int(rng.choice([r for r in LENGTHS if r >= 5]))
        tlen = rlen + 45
        alpha = int(rng.choice([1, 2, 2, 4, 4, 4]))
        if rng.random() < 0.4:
            per = int(rng.integers(1, 5)); base = np.tile(rng.integers(0, 4, per), tlen // per + 1)[:tlen]
        else:
            base = rng.integers(0, alpha, tlen)
        tx = B4[base]
        pos = int(rng.integers(0, 12))
        rs = tx[pos:pos + rlen].copy()
        nsub = int(rng.choice([0, 1, 2, 2, 2, 3, 3, 4]))
        places = rng.choice(rlen, size=min(nsub, rlen), replace=False)
        if rng.random() < 0.4 and rlen > 6: places = np.array([rlen - 1 - int(rng.integers(0, 3)), rlen - 1 - int(rng.integers(3, 6))])[:nsub]
        elif rng.random() < 0.2 and rlen > 6: places = np.array([int(rng.integers(0, 3)), int(rng.integers(3, 6))])[:nsub]
        rs = _sub(rng, rs, places)
        if rng.random() < 0.25 and rlen > 5:
            p = int(rng.integers(0, rlen - 1))
            rs = np.concatenate([rs[:p], rs[p + 1:], tx[pos + rlen:pos + rlen + 1]]) if rng.random() < 0.5 else np.concatenate([rs[:p], B4[rng.integers(0, 4, 1)], rs[p:-1]])
        out.append(_question(rng, rs, tx, pos, cs=REGULAR))


def paralogs(rng, out):
    """one 150-character segment in three transcripts at offsets of different residue mod 8, multi-mapping reads from it: equal target windows
    at different addresses"""
    seg = B4[rng.integers(0, 4, 150)]
    txs = [np.concatenate([B4[rng.integers(0, 4, o)], seg, B4[rng.integers(0, 4, 9)]]) for o in (0, 3, 13)]
    for rlen in (5, 8, 31, 64, 100, 129):
        for p in (0, 1, 17):
            for o, tx in zip((0, 3, 13), txs):
                for cs in (REGULAR, UNGAPPED):
                    rs = _sub(rng, seg[p:p + rlen], rng.choice(rlen, int(rng.integers(0, 3)), replace=False))
                    out.append(_question(rng, rs, tx, o + p, cs=cs, multi=True))


def questions(scheme):
    """the questions of a scheme, in an order that mixes the families (neighbouring groups of lanes then hold questions of different lengths and
    classes, and the strip tasks come four at a time with different lengths)"""
    rng = np.random.default_rng([7, scheme[0], -scheme[1], scheme[2], scheme[3], scheme[4] + 1])
    out = []
    substitutions(rng, out)
    many_differences(rng, out, 260)
    position_edges(rng, out, scheme)
    short_and_far(rng, out)
    odd_characters(rng, out, 300)
    loss_grid(rng, out, 400)
    scaled_losses(rng, out, scheme, 250, 320, 120)
    tiny_slices(rng, out)
    end_indels(rng, out, scheme, 160)
    clean_diagonal_thresholds(rng, out, scheme, 8)
    low_complexity(rng, out, 500)
    paralogs(rng, out)
    order = rng.permutation(len(out))
    return [out[i] for i in order]


Cases = collections.namedtuple("Cases", "scheme policy batch cls score geo ref wins")


@functools.lru_cache(maxsize=None)
def cases(scheme, policy=0):
    """the scheme's questions, classified and with their reference scores, computed once for the tests that share them.  policy 1 / 2: the
    questions whose position the Bowtie-2 policies turn down, and as many that they do not"""
    qs = questions(scheme)
    if policy:
        turned = [q for q in qs if geometry(q, policy).cls == "dropped"]
        qs = turned + [q for q in qs if geometry(q, policy).cls != "dropped"][:len(turned)]
    cls, score, geo, ref, wins = [], [], [], [], []
    for q in qs:
        c, s, roff, rlen, tlen1 = classify(q, policy, scheme)
        g = geometry(q, policy)
        cls.append(c); score.append(s); geo.append(g)
        r, wd = None, []
        if c == "ungapped":
            r = s
        elif c in ("known", "strip"):
            qq, tt = codes(q, g)
            r = ref_score(qq, tt, scheme)
            if c == "known":
                wd = winning_diagonals(qq, tt, scheme)
        ref.append(r); wins.append(wd)
    # a launch gets 256 / G questions per block and four strip tasks per wavefront: neither count a multiple, the last ones sit beside idle lanes
    drop = []
    if cls.count("strip") and cls.count("strip") % 4 == 0:
        drop.append(len(cls) - 1 - cls[::-1].index("strip"))
    if (len(qs) - len(drop)) % 128 == 0:
        drop.append(len(cls) - 1 - cls[::-1].index("ksw2"))
    for x in sorted(drop, reverse=True):
        for lst in (qs, cls, score, geo, ref, wins):
            del lst[x]
    return Cases(scheme, policy, Batch(qs), cls, score, geo, ref, wins)


def check_floors(cs):
    """on classify() alone, before any code under test runs: no class the scheme admits is left out"""
    diag, rule2, Ld, Li, strip = limits(cs.scheme)
    n = collections.Counter(cs.cls)
    assert n["ksw2"] >= 100 and n["ungapped"] >= 100 and n["off_end"] >= 10, n
    if diag:
        assert n["known"] >= 500, n
    if strip:
        assert n["strip"] >= 300, n
    if rule2:
        won = collections.Counter(d for c, s, r, wd in zip(cs.cls, cs.score, cs.ref, cs.wins) if c == "known" for d in wd)
        for d in list(range(1, Ld + 1)) + [-L for L in range(1, Li + 1)]:
            assert won[d] >= 100, (d, won)
    return n


# ---------------------------------------------------------------------------------------------------------------- what an answer must be
# (kind, tsc, key, task: what emu_sel.sel_side and probe.sel_side / sel_strip return; task rows are emu_sel.TASK_FIELDS)
_KIND = {"dropped": 0, "off_end": 0, "ungapped": 0, "known": 0, "strip": 6, "ksw2": 2}


def check_classes(cs, kind):
    """the class equals classify(): kind bit 1 (needs an alignment) and bit 2 (the strip kernel's) as the class says, bit 0 for a scored question
    of a multi-mapping unit"""
    bad = []
    for x, (q, c) in enumerate(zip(cs.batch.questions, cs.cls)):
        want = _KIND[c] | (1 if q.multi and c not in ("dropped", "off_end") else 0)
        if int(kind[x]) != want:
            bad.append((x, c, want, int(kind[x]), len(q.read), q.fwd, q.pos, len(q.tx), q.cs))
    assert not bad, "%d of %d questions in another class than classify() says, first (x, class, kind wanted, got, readLen, fwd, pos, tlen, cs): %r" % (len(bad), len(kind), bad[:5])


def check_tasks(cs, task):
    """a strip / ksw2 question leaves its SelTask -- the read, where the target window starts, roff, rlen, tlen1, fwd as the restatement has them --
    and nobody else writes one"""
    b = cs.batch
    bad = []
    for x, (q, c, g) in enumerate(zip(b.questions, cs.cls, cs.geo)):
        got = [int(v) for v in task[x]]
        if c in ("strip", "ksw2"):
            want = [1, int(b.roffs[x]), int(b.txp_off[b.qd[x][0]]) + g.pos, 2 * x, len(q.read), g.roff, g.rlen, g.tlen1, 1 if q.fwd else 0]
        else:
            want = [0] * 9
        if got != want:
            bad.append((x, c, want, got))
    assert not bad, "%d task records differ, first (x, class, wanted, got): %r" % (len(bad), bad[:5])


def check_scores(cs, tsc, strip_done):
    """every known and strip score is qo_ksw_extz2's, every ungapped score the plain count; dropped and off_end leave the lowest score, and so does a
    question that waits for its alignment (ksw2; strip before the strip pass)"""
    bad = []
    for x, (c, r) in enumerate(zip(cs.cls, cs.ref)):
        want = r if c in ("ungapped", "known") or (c == "strip" and strip_done) else LOWEST
        if int(tsc[x]) != want:
            q = cs.batch.questions[x]
            bad.append((x, c, want, int(tsc[x]), len(q.read), q.fwd, q.pos, len(q.tx)))
    assert not bad, "%d scores differ from the reference, first (x, class, wanted, got, readLen, fwd, pos, tlen): %r" % (len(bad), bad[:5])
    for x, (c, s, r) in enumerate(zip(cs.cls, cs.score, cs.ref)):      # (the restated rule itself, as test_ksw_variants.py holds it)
        assert c != "known" or s == r, (x, s, r)


def check_keys(cs, kind, key):
    """equal target windows with equal keyLen give equal keys, the distinct windows of the set distinct keys; no key without a multi-mapping unit"""
    by_window, n = {}, 0
    for x, (q, c, g) in enumerate(zip(cs.batch.questions, cs.cls, cs.geo)):
        if not q.multi or c in ("dropped", "off_end"):
            assert int(key[x]) == 0 and not int(kind[x]) & 1, (x, c, int(key[x]), int(kind[x]))
            continue
        by_window.setdefault((g.key_len, q.tx[g.pos:g.pos + g.key_len].tobytes()), set()).add(int(key[x])); n += 1
    assert n >= 500 and len(by_window) < n, (n, len(by_window))        # (keyed questions, and some of them share a window)
    split = [(k[0], sorted(v)) for k, v in by_window.items() if len(v) != 1]
    assert not split, "equal windows with different keys: %r" % split[:3]
    keys = [next(iter(v)) for v in by_window.values()]
    assert len(set(keys)) == len(keys), "distinct windows share a key"
