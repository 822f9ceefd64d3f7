"""The ksw2 extension kernel of the device source (rapmap_amd/csrc/qm_sel.inl: sel_ksw_extz2_rows, four alignments per
wavefront, one kernel for every --dpBandwidth -- run here through the lane emulation) against the oracle's restatement of
ksw_extz2_sse41 (oracle/qm_oracle.cpp: kswExtz2, itself checked against the reference's own ksw2 sources compiled into
oracle/_ref and against the reference's `-s` SAM fixtures), on random and adversarial inputs:
every target length 1..160 (all residues mod 16: the SSE vectors' padding lanes and the band's last rounds differ),
indels, N's, short and long queries, several bands and scoring schemes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.join(HERE, "emu"))
from oracle import oracle  # noqa: E402
import emu  # noqa: E402
import ksw_rows_cases as kc  # noqa: E402
from sel_side_cases import _known_answer_rule, _strip_dp  # noqa: E402  (the restatements of sel_side_score's rules and of sel_tasks_strip)


def _rows(el, grp, a, b, q_, e_, w, ring=-1):
    ql = (C.c_int * 4)(*[len(g[0]) for g in grp] + [0] * (4 - len(grp)))
    tl = (C.c_int * 4)(*[len(g[1]) for g in grp] + [0] * (4 - len(grp)))
    dummy = np.zeros(1, dtype=np.uint8)
    qp = (C.c_void_p * 4)(*[g[0].ctypes.data for g in grp] + [dummy.ctypes.data] * (4 - len(grp)))
    tp = (C.c_void_p * 4)(*[g[1].ctypes.data for g in grp] + [dummy.ctypes.data] * (4 - len(grp)))
    out = (C.c_int * 4)()
    el.qe_ksw_rows(ql, qp, tl, tp, a, b, q_, e_, w, out, ring)
    return list(out)


def rows(groups, scheme, ring=-1):
    """the lane emulation's row kernel, a wavefront (group) at a time (tests/ksw_rows_cases.py)"""
    el = emu._lib()
    return [_rows(el, grp, *scheme, ring)[:len(grp)] for grp in groups]


def rows8(groups, scheme):
    """... eight alignments of one shape per wavefront"""
    el = emu._lib()
    outs = []
    for grp in groups:
        n = len(grp)
        dummy = np.zeros(1, dtype=np.uint8)
        qp = (C.c_void_p * 8)(*[g[0].ctypes.data for g in grp] + [dummy.ctypes.data] * (8 - n))
        tp = (C.c_void_p * 8)(*[g[1].ctypes.data for g in grp] + [dummy.ctypes.data] * (8 - n))
        out = (C.c_int * 8)()
        el.qe_ksw_rows8(n, len(grp[0][0]), qp, len(grp[0][1]), tp, *scheme, out)
        outs.append(list(out)[:n])
    return outs


# the bodies of the row-kernel tests live in tests/ksw_rows_cases.py; test_ksw_rows_gpu.py runs them on the device
@pytest.mark.parametrize("scheme", kc.SCHEMES)
def test_ksw_rows_kernel_four_at_a_time(scheme):
    kc.four_at_a_time(rows, scheme)


@pytest.mark.parametrize("ring", kc.RINGS)
def test_ksw_rows_every_ring_gives_the_same_scores(ring):
    kc.every_ring_gives_the_same_scores(rows, ring)


@pytest.mark.parametrize("qmax", kc.QMAX)
def test_ksw_rows_longest_alignments(qmax):
    kc.longest_alignments(rows, qmax)


@pytest.mark.parametrize("w", kc.BANDS_EVERY_TLEN)
def test_ksw_rows_every_target_length(w):
    kc.every_target_length(rows, w)


@pytest.mark.parametrize("scheme", kc.SAME_SHAPE_SCHEMES)
def test_ksw_rows_same_shape_wavefronts(scheme):
    kc.same_shape_wavefronts(rows, scheme)


@pytest.mark.parametrize("scheme", kc.EIGHT_SCHEMES)
def test_ksw_rows_eight_per_wavefront(scheme):
    kc.eight_per_wavefront(rows8, scheme)


@pytest.mark.parametrize("scheme", [(2, -4, 4, 2, 15), (2, -4, 4, 2, 1), (2, -4, 4, 2, 5), (1, -1, 1, 1, 15), (2, -6, 5, 3, 33), (4, -4, 6, 2, 20),
                                    (2, -4, 4, 2, 98), (2, -4, 4, 2, -1), (3, -2, 2, 1, 15), (1, 0, 25, 25, 15)])
def test_gapless_path_wins_when_it_loses_no_more_than_one_gap(scheme):
    """sel_side_score's first rule (rapmap_amd/csrc/qm_sel.inl): with the target at least as long as the query, an extension alignment
    whose gapless path loses at most q + e against 'every query character at its best' scores exactly what that path scores.
    Held against the oracle's ksw_extz2 (itself pinned to the reference's kernel compiled in place) on queries with zero, one or
    two differences, N's on either side, indels right behind the start, every length class and band (but --dpBandwidth 0, whose
    odd anti-diagonals are empty: the kernel stops at the second one, and the shortcut stays away from it)."""
    a, b, q_, e_, w = scheme
    ol = oracle._lib()
    ol.qo_ksw_extz2.restype = C.c_int
    rng = np.random.default_rng(1234 + w)
    hits = 0
    for it in range(4000):
        qlen = int(rng.integers(1, 141))
        tlen = qlen + int(rng.integers(0, 25))
        q = rng.integers(0, 4, qlen).astype(np.uint8)
        t = np.concatenate([q, rng.integers(0, 4, tlen - qlen).astype(np.uint8)])
        for _ in range(int(rng.integers(0, 3))):              # substitutions in the target
            t[rng.integers(0, qlen)] = rng.integers(0, 4)
        if rng.random() < 0.15: q[rng.integers(0, qlen)] = 4  # an N in the query
        if rng.random() < 0.15: t[rng.integers(0, tlen)] = 4  # ... in the target
        if rng.random() < 0.1 and qlen > 4:                   # a deletion: the target continues one character further on
            p = int(rng.integers(0, qlen - 1)); t = np.concatenate([t[:p], t[p + 1:], rng.integers(0, 4, 1).astype(np.uint8)])
        aa, bb = abs(a), -abs(b)
        sc = np.where((q < 4) & (t[:qlen] < 4), np.where(q == t[:qlen], aa, bb), 0)
        smax = int(np.where(q < 4, aa, 0).sum()); U = int(sc.sum())
        if smax - U <= q_ + e_:
            ref = ol.qo_ksw_extz2(qlen, q.ctypes.data_as(C.c_void_p), len(t), t.ctypes.data_as(C.c_void_p), a, b, q_, e_, w)
            assert ref == U, (scheme, qlen, tlen, smax, U, ref)
            hits += 1
    assert hits > 500


@pytest.mark.parametrize("scheme", [(2, -4, 5, 3, 15), (2, -4, 4, 2, 15), (2, -4, 4, 2, 8), (1, -1, 1, 1, 15), (2, -6, 5, 3, 33), (4, -4, 6, 2, 20),
                                    (2, -4, 4, 2, -1), (3, -2, 2, 1, 15), (2, -4, 5, 3, 9), (1, -3, 2, 1, 15), (2, -4, 6, 1, 15)])
def test_two_mismatches_lose_to_at_most_one_gap_run(scheme):
    """sel_side_score's second rule (rapmap_amd/csrc/qm_sel.inl), restated above in numpy: an alignment whose gapless path has exactly
    two mismatches and no N scores the best of that path and the one-gap-run paths without a mismatch -- found by looking at the last
    mismatch of the diagonals next to the main one.  Held against the oracle's ksw_extz2 on queries from low-complexity and periodic
    targets (where the neighbouring diagonals do match), with the substitutions at the ends, true indels, N's."""
    a, b, q_, e_, w = scheme
    ol = oracle._lib()
    ol.qo_ksw_extz2.restype = C.c_int
    rng = np.random.default_rng(7 + w + q_)
    tot = ext = gapwin = 0
    for it in range(6000):
        qlen = int(rng.integers(3, 141))
        tlen = qlen + int(rng.integers(0, 25))
        alpha = int(rng.choice([1, 2, 2, 4, 4, 4]))
        if rng.random() < 0.3:
            per = int(rng.integers(1, 4)); unit = rng.integers(0, 4, per)
            base = np.tile(unit, (tlen + 8) // per + 1)[:tlen + 8].astype(np.uint8)
        else:
            base = rng.integers(0, alpha, tlen + 8).astype(np.uint8)
        t = base[:tlen].copy(); q = base[:qlen].copy()
        nsub = int(rng.choice([2, 2, 2, 1, 3]))
        pos = rng.choice(qlen, size=min(nsub, qlen), replace=False)
        if rng.random() < 0.4 and qlen > 6: pos = np.array([qlen - 1 - int(rng.integers(0, 3)), qlen - 1 - int(rng.integers(3, 6))])[:nsub]
        if rng.random() < 0.2 and qlen > 6: pos = np.array([int(rng.integers(0, 3)), int(rng.integers(3, 6))])[:nsub]
        for p in pos: q[p] = (q[p] + 1 + rng.integers(0, 3)) % 4
        if rng.random() < 0.15 and qlen > 5:
            p = int(rng.integers(0, qlen - 1))
            if rng.random() < 0.5: q = np.concatenate([q[:p], q[p + 1:], base[qlen:qlen + 1]])
            else: q = np.concatenate([q[:p], rng.integers(0, 4, 1).astype(np.uint8), q[p:-1]])
        if rng.random() < 0.03: q[rng.integers(0, qlen)] = 4
        if rng.random() < 0.03: t[rng.integers(0, tlen)] = 4
        r = _known_answer_rule(q, t, a, b, q_, e_, w)
        if r is None: continue
        ref = ol.qo_ksw_extz2(qlen, q.ctypes.data_as(C.c_void_p), len(t), t.ctypes.data_as(C.c_void_p), a, b, q_, e_, w)
        assert r == ref, (scheme, qlen, tlen, r, ref, q.tolist(), t.tolist())
        tot += 1
        aa, bb = abs(a), -abs(b)
        U = int(np.where((q < 4) & (t[:qlen] < 4), np.where(q == t[:qlen], aa, bb), 0).sum())
        if int(np.where(q < 4, aa, 0).sum()) - U > q_ + e_:
            ext += 1; gapwin += r != U
    M = abs(a) + abs(b)
    if M <= q_ + e_: assert tot > 1000
    if M <= q_ + e_ and (w < 0 or w >= 8) and q_ + 4 * e_ >= 2 * M and q_ + 3 * (e_ + abs(a)) >= 2 * M:   # (the rule's own limits)
        assert ext > 300 and gapwin > 0, (tot, ext, gapwin)


@pytest.mark.parametrize("scheme", [(2, -4, 4, 2, 15), (2, -4, 5, 3, 15), (1, -1, 1, 1, 15), (2, -6, 5, 3, 33), (2, -4, 4, 2, -1), (3, -2, 2, 1, 15), (2, -4, 6, 1, 15)])
def test_strip_dp_equals_ksw2_when_the_gapless_path_is_close(scheme):
    """sel_tasks_strip (rapmap_amd/csrc/qm_sel.inl), restated above: the extension alignment as a plain affine-gap recurrence over the
    diagonals -7 .. +8.  When the gapless path loses no more than q + 7 e no path that scores as much leaves that strip, so the strip's
    maximum over the query's last row and the target's last column is ksw_extz2's score -- held against the oracle's kernel on
    periodic / low-complexity targets, substitutions, true indels, N's and targets that end right behind the query."""
    a, b, go, ge, w = scheme
    ol = oracle._lib()
    ol.qo_ksw_extz2.restype = C.c_int
    rng = np.random.default_rng(3 + go + w)
    used = 0
    for it in range(2500):
        qlen = int(rng.integers(3, 141)); tlen = qlen + int(rng.integers(0, 25))
        alpha = int(rng.choice([1, 2, 4, 4, 4]))
        if rng.random() < 0.3:
            per = int(rng.integers(1, 4)); unit = rng.integers(0, 4, per); base = np.tile(unit, (tlen + 8) // per + 1)[:tlen + 8].astype(np.uint8)
        else:
            base = rng.integers(0, alpha, tlen + 8).astype(np.uint8)
        t = base[:tlen].copy(); q = base[:qlen].copy()
        for p in rng.choice(qlen, size=min(int(rng.integers(0, 5)), qlen), replace=False): q[p] = (q[p] + 1 + rng.integers(0, 3)) % 4
        if rng.random() < 0.3 and qlen > 5:
            p = int(rng.integers(0, qlen - 1))
            if rng.random() < 0.5: q = np.concatenate([q[:p], q[p + 1:], base[qlen:qlen + 1]])
            else: q = np.concatenate([q[:p], rng.integers(0, 4, 1).astype(np.uint8), q[p:-1]])
        if rng.random() < 0.1: q[rng.integers(0, qlen)] = 4
        if rng.random() < 0.1: t[rng.integers(0, tlen)] = 4
        aa, bb = abs(a), -abs(b)
        sc = np.where((q < 4) & (t[:qlen] < 4), np.where(q == t[:qlen], aa, bb), 0)
        loss = int(np.where(q < 4, aa, 0).sum()) - int(sc.sum())
        if not (tlen >= qlen and loss <= go + 7 * ge and (w < 0 or w >= 9) and aa - bb + go + ge <= 96): continue
        used += 1
        r = _strip_dp(q.tolist(), t.tolist(), a, b, go, ge)
        ref = ol.qo_ksw_extz2(qlen, q.ctypes.data_as(C.c_void_p), len(t), t.ctypes.data_as(C.c_void_p), a, b, go, ge, w)
        assert r == ref, (scheme, qlen, tlen, loss, r, ref, q.tolist(), t.tolist())
    assert used > 500
