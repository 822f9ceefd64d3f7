"""Inputs of the ksw2 row-kernel tests (test_ksw_variants.py: lane emulation, test_ksw_rows_gpu.py: device): sel_ksw_extz2_rows<RING>, four
alignments per wavefront, and the register edition's eight-per-wavefront form (rapmap_amd/csrc/qm_sel.inl), against the oracle's restatement of
ksw_extz2_sse41 (oracle/qm_oracle.cpp: qo_ksw_extz2).

Every body is a function of two callables:
    rows(groups, scheme, ring)  groups: [[(query, target) x 1 .. 4]] nt4 code arrays, one group per wavefront, the rows a group leaves out idle;
                                scheme: (match, mismatch, gap open, gap extend, band); ring: 32 / 64 / 128 / 1024 slots, -1: what the launch
                                wrapper picks for the band -> [[score per alignment]]
    rows8(groups, scheme)       groups of 1 .. 8 alignments of ONE shape -> [[score per alignment]]
A body hands all the groups of a scheme over in one call."""
import ctypes as C

import numpy as np

from oracle import oracle
from parity_cases import ksw_cases, ksw_mutate

# (match, mismatch, gap open, gap extend, band): bands <= 15 run on the register edition of the row kernel ("32"), <= 33 on the
# 64-slot ring, <= 97 on 128 slots, everything else (and the "whole matrix" band -1) on 1024
SCHEMES = [(2, -4, 4, 2, 15), (2, -4, 4, 2, 5), (1, -1, 1, 1, 15), (2, -6, 5, 3, 33), (2, -4, 4, 2, 0), (4, -4, 6, 2, 20),
           (2, -4, 4, 2, 1), (2, -6, 5, 3, 8), (1, 0, 25, 25, 15), (2, -4, 4, 2, 14), (2, -4, 4, 2, 16),
           (2, -4, 4, 2, 34), (2, -4, 4, 2, 40), (2, -6, 5, 3, 64), (1, -1, 1, 1, 97), (2, -4, 4, 2, 98), (2, -4, 4, 2, 150),
           (2, -4, 4, 2, 1000), (2, -4, 4, 2, -1)]
RINGS = [32, 64, 128, 1024]
QMAX = [256, 512]
BANDS_EVERY_TLEN = [15, 40, 120]
SAME_SHAPE_SCHEMES = [(2, -4, 4, 2, 15), (2, -6, 5, 3, 8), (1, -1, 1, 1, 0), (2, -4, 4, 2, 5), (1, 0, 25, 25, 15)]
EIGHT_SCHEMES = [(2, -4, 4, 2, 15), (2, -6, 5, 3, 8), (1, -1, 1, 1, 0), (2, -4, 4, 2, 5)]


def ref_score(qq, tt, scheme):
    """the oracle's ksw_extz2 (the plain CPU reference the emulation is held to)"""
    a, b, q_, e_, w = scheme
    ol = oracle._lib()
    ol.qo_ksw_extz2.restype = C.c_int
    return ol.qo_ksw_extz2(len(qq), qq.ctypes.data_as(C.c_void_p), len(tt), tt.ctypes.data_as(C.c_void_p), a, b, q_, e_, w)


def four_at_a_time(rows, scheme):
    """the 16-lane-row kernel (four alignments of different shapes per wavefront, idle rows included) against the oracle"""
    w = scheme[4]
    cases = list(ksw_cases(4321 + w, 400))
    rng = np.random.default_rng(5)
    groups = []
    for i in range(0, len(cases), 4):
        grp = cases[i:i + 4]
        if rng.random() < 0.2:
            grp = grp[:int(rng.integers(1, 4))]            # a partly filled wavefront
        groups.append(grp)
    outs = rows(groups, scheme, -1)
    bad = []
    for grp, out in zip(groups, outs):
        for k, (qq, tt) in enumerate(grp):
            ref = ref_score(qq, tt, scheme)
            if out[k] != ref:
                bad.append((k, len(qq), len(tt), ref, out[k]))
    assert not bad, "%d mismatches, first: %r" % (len(bad), bad[:5])


def every_ring_gives_the_same_scores(rows, ring):
    """a band that fits the smallest ring must score the same on the larger ones (the ring is storage, not arithmetic); 32: the
    register edition, bands up to 15 only"""
    cases = list(ksw_cases(99, 200))
    groups = [cases[i:i + 4] for i in range(0, len(cases), 4)]
    for w in ((15, 7) if ring == 32 else (15, 33)):
        scheme = (2, -4, 4, 2, w)
        outs = rows(groups, scheme, ring)
        for grp, out in zip(groups, outs):
            for k, (qq, tt) in enumerate(grp):
                ref = ref_score(qq, tt, scheme)
                assert out[k] == ref, (ring, w, len(qq), len(tt), ref, out[k])


def longest_alignments(rows, qmax):
    """queries of up to 512 bases against targets 20 longer (the longest the -s path produces), narrow to full band"""
    rng = np.random.default_rng(31 + qmax)
    for w in (15, 33, 60, 97, 200, -1):
        scheme = (2, -4, 4, 2, w)
        grp = []
        for _ in range(4):
            q = rng.integers(0, 4, int(rng.integers(qmax - 26, qmax + 1))).astype(np.uint8)
            t = ksw_mutate(rng, q, len(q) + 20, sub=0.03, indel=0.01)
            grp.append((q, t))
        out = rows([grp], scheme, -1)[0]
        for k, (qq, tt) in enumerate(grp):
            ref = ref_score(qq, tt, scheme)
            assert out[k] == ref, (w, len(qq), len(tt), ref, out[k])


def every_target_length(rows, w):
    """query 100, perfect and 1-error targets of every length 1..160: the rounds where the band has shrunk to its last cells
    sit at a different place of the 16-byte vectors for every residue of tlen mod 16"""
    scheme = (2, -4, 4, 2, w)
    rng = np.random.default_rng(9)
    groups = []
    for t0 in range(1, 161, 4):
        grp = []
        for tlen in range(t0, t0 + 4):
            q = rng.integers(0, 4, 100).astype(np.uint8)
            t = np.resize(q, tlen).copy()
            if tlen > 3:
                t[tlen // 2] ^= 1
            grp.append((q, t))
        groups.append(grp)
    outs = rows(groups, scheme, -1)
    for grp, out in zip(groups, outs):
        for k in range(4):
            qq, tt = grp[k]
            ref = ref_score(qq, tt, scheme)
            assert out[k] == ref, (w, len(tt), ref, out[k])


def _one_shape_groups(rng, shapes, sizes):
    groups = []
    for qlen, tlen in shapes:
        for n in sizes(rng):
            grp = []
            for _ in range(n):
                q = rng.integers(0, 4, qlen).astype(np.uint8)
                if rng.random() < 0.2:
                    q[rng.integers(0, qlen)] = 4
                t = ksw_mutate(rng, q, tlen) if rng.random() < 0.85 else rng.integers(0, 5, tlen).astype(np.uint8)
                grp.append((q, t))
            groups.append(grp)
    return groups


def _compare(groups, outs, scheme):
    bad = []
    for grp, out in zip(groups, outs):
        for k, (qq, tt) in enumerate(grp):
            ref = ref_score(qq, tt, scheme)
            if out[k] != ref:
                bad.append((k, len(grp), len(qq), len(tt), ref, out[k]))
    assert not bad, "%d mismatches, first: %r" % (len(bad), bad[:5])


def same_shape_wavefronts(rows, scheme):
    """four (or fewer: idle rows) alignments of ONE shape per wavefront -- the register edition then keeps the band's geometry on
    the scalar unit (sel_ksw_extz2_rows_reg<.., UNI = true>): every query length class and target length residue, indels, N's"""
    rng = np.random.default_rng(77 + scheme[4])
    shapes = [(100, 120), (100, 100), (100, 87), (1, 1), (1, 21), (31, 51), (75, 95), (140, 160), (50, 1), (16, 16), (17, 33), (128, 148)]
    shapes += [(int(rng.integers(1, 141)), int(rng.integers(1, 161))) for _ in range(60)]
    groups = _one_shape_groups(rng, shapes, lambda r: (4, 4, int(r.integers(1, 4))))
    _compare(groups, rows(groups, scheme, -1), scheme)


def eight_per_wavefront(rows8, scheme):
    """eight alignments of one shape as two sets of state through the same rounds (sel_ksw_extz2_rows_reg<.., UNI, 2>, what
    qm_sel_align2_kernel runs when a wavefront's eight tasks share their lengths), 5 .. 8 of them real"""
    rng = np.random.default_rng(177 + scheme[4])
    shapes = [(100, 120), (100, 100), (100, 87), (1, 1), (31, 51), (75, 95), (140, 160), (16, 16), (17, 33), (128, 148)]
    shapes += [(int(rng.integers(1, 141)), int(rng.integers(1, 161))) for _ in range(40)]
    groups = _one_shape_groups(rng, shapes, lambda r: (8, int(r.integers(5, 8))))
    _compare(groups, rows8(groups, scheme), scheme)
