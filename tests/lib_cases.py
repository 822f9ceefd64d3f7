"""Inputs, the restatement and the checks of the library-type tests (test_lib_format.py: lane emulation and the host functions,
test_lib_format_gpu.py: device).  Everything here is exact: integer tallies, offsets and tid lists.

codes() restates the code table of include/qmap_mi355.h in numpy, tally() the 32 words and the filtered lists, infer() the
inference in Python integers, filtered_classes() the label -> count dictionary of the filtered lists.  A check takes
`new(lib_type, max_blocks)`, which makes an object with add_hits / compact_hits / add_counts / counts / stat / clear / close --
rapmap_amd.LibFormat on the device, emu_lib.EmuLib under the lane emulation; lib_type is a type name or a mask."""
import numpy as np

from rapmap_amd.api import HIT_DTYPE

CODES = ("ISF", "ISR", "OSF", "OSR", "MSF", "MSR", "LF", "LR", "RF", "RR", "SF", "SR")
ISF, ISR, OSF, OSR, MSF, MSR, LF, LR, RF, RR, SF, SR, OTHER = range(13)
ALL_CODES = 0xfff
TYPES = {"IU": (ISF, ISR, LF, LR, RF, RR), "ISF": (ISF, LF, RR), "ISR": (ISR, LR, RF),
         "OU": (OSF, OSR, LF, LR, RF, RR), "OSF": (OSF, LF, RR), "OSR": (OSR, LR, RF),
         "MU": (MSF, MSR, LF, LR, RF, RR), "MSF": (MSF, LF, RF), "MSR": (MSR, LR, RR),
         "U": (SF, SR), "SF": (SF,), "SR": (SR,), "A": tuple(range(12))}
W_SINGLE, W_UNITS, W_UNMAPPED, W_KEPT, W_DROPPED, W_HITS, W_KEPT_HITS, W_OTHER = 12, 24, 25, 26, 27, 28, 29, 30


def mask_of(lib_type):
    """the 12-bit mask of a type name; a number is taken as a mask"""
    if isinstance(lib_type, str):
        return sum(1 << c for c in TYPES[lib_type])
    return int(lib_type)


def codes(hits):
    """int64[len(hits)]: the code of every record, 12 for `other`; a byte counts as forward when it is not 0, positions are signed"""
    h = np.asarray(hits)
    f = h["fwd"] != 0; mf = h["mate_is_fwd"] != 0; ms = h["mate_status"].astype(np.int64)
    pos = h["pos"].astype(np.int64); mpos = h["mate_pos"].astype(np.int64)
    outward = (f & (pos > mpos)) | (mf & (mpos > pos))
    rev = (~f).astype(np.int64)
    c = np.full(h.size, OTHER, dtype=np.int64)
    paired = ms == 3
    opp = paired & (f != mf)
    c[opp] = (np.where(outward, OSF, ISF) + rev)[opp]
    c[paired & f & mf] = MSF; c[paired & ~f & ~mf] = MSR
    c[ms == 1] = (LF + rev)[ms == 1]; c[ms == 2] = (RF + rev)[ms == 2]; c[ms == 0] = (SF + rev)[ms == 0]
    return c


def tally(hit_offsets, hits, lib_type):
    """-> (counts uint64[32], new_offsets int64[n + 1], tids uint32[]): the 32 words and the filtered lists"""
    mask = mask_of(lib_type)
    off = np.asarray(hit_offsets, dtype=np.int64)
    n = len(off) - 1
    base = int(off[0]) if n >= 0 else 0
    h = np.asarray(hits)[base:int(off[-1])] if hits is not None and len(hits) else np.zeros(0, dtype=HIT_DTYPE)
    off = off - base
    c = codes(h)
    keep = (c < 12) & (((mask >> np.minimum(c, 12)) & 1) != 0)
    w = np.zeros(32, dtype=np.uint64)
    w[:12] = np.bincount(c, minlength=13)[:12]
    w[W_OTHER] = int(np.count_nonzero(c == OTHER)); w[W_HITS] = h.size; w[W_KEPT_HITS] = int(keep.sum())
    cum = np.zeros(h.size + 1, dtype=np.int64); np.cumsum(keep, out=cum[1:])
    new_off = cum[off]
    cnt = np.diff(off); kc = np.diff(new_off)
    w[W_UNITS] = n; w[W_UNMAPPED] = int(np.count_nonzero(cnt == 0))
    w[W_KEPT] = int(np.count_nonzero(kc > 0)); w[W_DROPPED] = int(np.count_nonzero((cnt > 0) & (kc == 0)))
    one = c[off[:-1][cnt == 1]]
    w[W_SINGLE:W_SINGLE + 12] = np.bincount(one, minlength=13)[:12]
    assert_invariants(w, mask)
    return w, new_off, h["tid"][keep].astype(np.uint32)


def assert_invariants(w, lib_type, what=""):
    mask = mask_of(lib_type)
    w = [int(x) for x in w]
    assert sum(w[:12]) + w[W_OTHER] == w[W_HITS], what
    assert w[W_UNMAPPED] + w[W_KEPT] + w[W_DROPPED] == w[W_UNITS], what
    assert w[W_KEPT_HITS] == sum(w[c] for c in range(12) if (mask >> c) & 1), what
    assert w[31] == 0, what


def infer(counts):
    """the expected type from words [12..23], in Python integers"""
    s = [int(x) for x in counts[W_SINGLE:W_SINGLE + 12]]
    assert all(x < 2 ** 59 for x in s)
    orient = [("I", s[ISF], s[ISR]), ("O", s[OSF], s[OSR]), ("M", s[MSF], s[MSR]), ("", s[SF], s[SR])]
    best = orient[0]
    for o in orient[1:]:
        if o[1] + o[2] > best[1] + best[2]:
            best = o
    name, a, b = best
    if a + b == 0:
        return ""
    return name + ("SF" if 10 * a > 7 * (a + b) else "SR" if 10 * a < 3 * (a + b) else "U")


def filtered_classes(new_off, tids):
    """{label: count} of the filtered lists: a label is the ascending tuple of a list's distinct tids; empty lists contribute nothing"""
    d = {}
    for u in range(len(new_off) - 1):
        a, b = int(new_off[u]), int(new_off[u + 1])
        if b > a:
            k = tuple(sorted(set(int(t) for t in tids[a:b])))
            d[k] = d.get(k, 0) + 1
    return d


def table_classes(label_offsets, tids, counts):
    """what EqClasses.fetch gives, as the same kind of dictionary"""
    return {tuple(int(t) for t in tids[int(label_offsets[i]):int(label_offsets[i + 1])]): int(counts[i]) for i in range(len(counts))}


# ---- case builders

FWD_BYTES = np.array([1, 2, 255], dtype=np.uint8)


def records(want, rng, n_txps=50):
    """hit records whose codes are `want` (12: other), random in every field the sweep must not look at; forward bytes are 1, 2 or
    255, positions go below 0 and every fifth record has pos == mate_pos where its code allows it"""
    want = np.asarray(want, dtype=np.int64)
    n = want.size
    h = np.zeros(n, dtype=HIT_DTYPE)
    h["tid"] = rng.integers(0, n_txps, n)
    h["frag_len"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    h["read_len"] = rng.integers(0, 300, n); h["mate_len"] = rng.integers(0, 300, n)
    h["is_paired"] = rng.integers(0, 256, n); h["aln_score"] = rng.integers(-100, 100, n)
    pos = rng.integers(-60, 5000, n); d = rng.integers(1, 400, n)
    eq = (np.arange(n) % 5) == 0
    fb = rng.choice(FWD_BYTES, n)
    h["pos"] = pos; h["mate_pos"] = rng.integers(-60, 5000, n)
    h["fwd"] = rng.integers(0, 2, n) * fb; h["mate_is_fwd"] = rng.integers(0, 2, n) * rng.choice(FWD_BYTES, n)
    for c in range(13):
        i = np.flatnonzero(want == c)
        if not i.size:
            continue
        if c <= OSR:
            h["mate_status"][i] = 3
            fwd = c in (ISF, OSF)
            h["fwd"][i] = fb[i] if fwd else 0; h["mate_is_fwd"][i] = 0 if fwd else fb[i]
            if c == ISF:       # not outward: pos <= mate_pos
                h["mate_pos"][i] = np.where(eq[i], pos[i], pos[i] + d[i])
            elif c == ISR:     # not outward: mate_pos <= pos
                h["mate_pos"][i] = np.where(eq[i], pos[i], pos[i] - d[i])
            elif c == OSF:     # pos > mate_pos
                h["mate_pos"][i] = pos[i] - d[i]
            else:              # mate_pos > pos
                h["mate_pos"][i] = pos[i] + d[i]
        elif c in (MSF, MSR):
            h["mate_status"][i] = 3
            h["fwd"][i] = fb[i] if c == MSF else 0; h["mate_is_fwd"][i] = rng.choice(FWD_BYTES, i.size) if c == MSF else 0
            h["mate_pos"][i] = np.where(eq[i], pos[i], h["mate_pos"][i])
        elif c < OTHER:
            h["mate_status"][i] = {LF: 1, LR: 1, RF: 2, RR: 2, SF: 0, SR: 0}[c]
            h["fwd"][i] = fb[i] if c in (LF, RF, SF) else 0
        else:
            h["mate_status"][i] = rng.choice(np.array([4, 7, 128, 255], dtype=np.uint8), i.size)
    assert np.array_equal(codes(h), want)                            # the restatement gives every crafted code back
    return h


def offsets_of(sizes):
    off = np.zeros(len(sizes) + 1, dtype=np.int64); np.cumsum(np.asarray(sizes, dtype=np.int64), out=off[1:])
    return off


UNIT_SIZES = (0, 1, 2, 8, 9, 64, 65, 200)


def sizes_for(total, rng):
    """unit sizes out of UNIT_SIZES (every one that fits at least once, then at random) that add up to exactly `total` hits"""
    sizes = []; left = total
    for s in UNIT_SIZES:
        if s <= left:
            sizes.append(s); left -= s
    while left > 0:
        s = int(rng.choice([x for x in UNIT_SIZES if 0 < x <= left]))
        sizes.append(s); left -= s
        if rng.integers(0, 3) == 0:
            sizes.append(0)
    sizes = list(rng.permutation(np.asarray(sizes + [0], dtype=np.int64)))
    assert sum(sizes) == total
    return sizes


def random_codes(n, rng, every_wave=True):
    """n codes at random; with every_wave the first thirteen hits of every full 64 hold the twelve codes and `other`"""
    c = rng.integers(0, 13, n)
    if every_wave:
        for b in range(0, n - 63, 64):
            c[b:b + 13] = rng.permutation(13)
    return c


def random_batch(total, seed, sizes=None, every_wave=True):
    rng = np.random.default_rng(seed)
    sizes = sizes_for(total, rng) if sizes is None else sizes
    return offsets_of(sizes), records(random_codes(int(sum(sizes)), rng, every_wave), rng)


def sweep_once(new, off, hits, lib_type, max_blocks=0):
    """(counts of add_hits, (counts, new_offsets, tids) of compact_hits) from two fresh objects"""
    a = new(lib_type, max_blocks); b = new(lib_type, max_blocks)
    try:
        a.add_hits(off, hits)
        no, t = b.compact_hits(off, hits)
        return a.counts(), (b.counts(), no, t)
    finally:
        a.close(); b.close()


def assert_same(got, exp, lib_type, what):
    got = np.asarray(got, dtype=np.uint64)
    assert np.array_equal(got, exp), "%s: tallies differ: %r, expected %r" % (what, got.tolist(), exp.tolist())
    assert_invariants(got, lib_type, what)


def check_against_restatement(new, off, hits, lib_type, max_blocks=0, what=""):
    ew, eo, et = tally(off, hits, lib_type)
    ca, (cb, no, t) = sweep_once(new, off, hits, lib_type, max_blocks)
    what = "%s, %s" % (what, lib_type)
    assert_same(ca, ew, lib_type, what + " (add_hits)"); assert_same(cb, ew, lib_type, what + " (compact_hits)")
    assert np.array_equal(no, eo), what + ": new offsets differ"
    assert np.array_equal(t, et), what + ": tids differ"
    return ew, eo, et


# ---- the crafted checks, by name; each the smallest shape at which that part of the sweep can still go wrong

HIT_TOTALS = (0, 1, 63, 64, 65, 127, 128, 129, 4097)
SINGLE_MASKS = tuple(1 << c for c in range(12))


def check_sizes(new):
    for total in HIT_TOTALS:
        off, h = random_batch(total, seed=200 + total)
        for t in ("IU", "ISF", "A"):
            ew, _, _ = check_against_restatement(new, off, h, t, what="%d hits" % total)
        if total == 4097:
            assert set(np.diff(off).tolist()) == set(UNIT_SIZES)     # units of 0, 1, 2, 8, 9, 64, 65 and 200 hits
            c = codes(h)
            for b in range(0, total - 63, 64):
                assert set(c[b:b + 64].tolist()) == set(range(13)), b   # every code, `other` too, in every wavefront
            assert all(int(x) > 0 for x in ew[:12]) and int(ew[W_OTHER]) > 0


def check_wave_boundaries(new):
    # a unit that ends at lane 62, one that begins at lane 63, one that begins at lane 0 and spans three wavefronts, empty units between
    # them, a unit from lane 63 on over three wavefronts, and a last one that ends in the middle of a wavefront
    sizes = [63, 0, 1, 0, 130, 61, 0, 66, 5]
    off = offsets_of(sizes)
    assert off[2] % 64 == 63 and off[4] % 64 == 0 and (off[5] - 1) // 64 - off[4] // 64 == 2 and off[7] % 64 == 63 and (off[8] - 1) // 64 - off[7] // 64 == 2
    rng = np.random.default_rng(3)
    h = records(random_codes(int(off[-1]), rng), rng)
    for t in sorted(TYPES) + list(SINGLE_MASKS):
        check_against_restatement(new, off, h, t, what="wave boundaries")


def check_code_edges(new):
    """pos == mate_pos on both strands, negative positions, forward bytes of 2 and 255, mate_status beyond 3"""
    h = np.zeros(12, dtype=HIT_DTYPE)
    h["mate_status"] = 3
    h["fwd"] = [2, 0, 255, 0, 1, 0, 2, 255, 0, 0, 1, 0]; h["mate_is_fwd"] = [0, 255, 0, 2, 0, 1, 0, 0, 2, 255, 0, 1]
    h["pos"] = [7, 7, -5, -5, -3, -9, -9, 0, 0, -1, -2147483648, 2147483647]
    h["mate_pos"] = [7, 7, -5, -5, -9, -3, -3, -1, -1, 0, 2147483647, -2147483648]
    exp = [ISF, ISR, ISF, ISR, OSF, OSR, ISF, OSF, ISR, OSR, ISF, ISR]
    assert codes(h).tolist() == exp
    extra = np.zeros(6, dtype=HIT_DTYPE)
    extra["mate_status"] = [4, 255, 3, 3, 0, 2]; extra["fwd"] = [1, 0, 2, 0, 255, 2]; extra["mate_is_fwd"] = [0, 1, 255, 0, 7, 0]
    h = np.concatenate([h, extra])
    assert codes(h).tolist() == exp + [OTHER, OTHER, MSF, MSR, SF, RF]
    for off in (np.arange(19), offsets_of([18]), offsets_of([3, 0, 15])):
        for t in ("IU", "ISF", "ISR", "OSF", "OSR", "A", "U"):
            check_against_restatement(new, off, h, t, what="code edges")


def check_masks(new):
    off, h = random_batch(1000, seed=5)
    for t in sorted(TYPES) + list(SINGLE_MASKS):
        ew, _, _ = check_against_restatement(new, off, h, t, what="1000 hits")
        assert int(ew[W_KEPT_HITS]) > 0


def check_keep_patterns(new):
    """all / none / alternating / only lane 63 / only lane 0 of every wavefront kept, under a mask of one code"""
    n = 64 * 5 + 17
    lane = np.arange(n) % 64
    rng = np.random.default_rng(9)
    off = offsets_of(sizes_for(n, rng))
    for name, keep in (("all", lane >= 0), ("none", lane < 0), ("alternating", lane % 2 == 0), ("lane 63", lane == 63), ("lane 0", lane == 0)):
        for kept_code, other_code in ((ISF, ISR), (RR, OTHER)):
            h = records(np.where(keep, kept_code, other_code), rng)
            ew, eo, et = check_against_restatement(new, off, h, 1 << kept_code, what="keep " + name)
            assert int(ew[W_KEPT_HITS]) == int(keep.sum()) == et.size


def check_partly_filtered(new):
    """units whose hits are partly compatible: the kept ones in their order; a tid whose first occurrence is dropped and whose second is
    kept; a unit of 200 hits that keeps one"""
    rng = np.random.default_rng(11)
    want = [ISR, ISF, ISF, ISR,          # unit 0: the two in the middle
            ISR, ISF,                     # unit 1: tid 7 twice, the first dropped
            ISF, ISR, OTHER,              # unit 2: the first
            ISR, LR]                      # unit 3: nothing under ISF
    sizes = [4, 2, 3, 2, 200, 0, 1]
    big = [ISR] * 200; big[137] = ISF
    want = want + big + [LF]
    h = records(want, rng)
    h["tid"][:11] = [1, 2, 3, 4, 7, 7, 5, 6, 6, 8, 9]
    h["tid"][11:211] = 20; h["tid"][11 + 137] = 21; h["tid"][211] = 30
    off = offsets_of(sizes)
    ew, eo, et = check_against_restatement(new, off, h, "ISF", what="partly filtered")
    assert eo.tolist() == [0, 2, 3, 4, 4, 5, 5, 6] and et.tolist() == [2, 3, 7, 5, 21, 30]
    assert (int(ew[W_KEPT]), int(ew[W_DROPPED]), int(ew[W_UNMAPPED])) == (5, 1, 1)
    assert filtered_classes(eo, et) == {(2, 3): 1, (7,): 1, (5,): 1, (21,): 1, (30,): 1}
    for t in ("ISR", "IU", "A", 1 << LR):
        check_against_restatement(new, off, h, t, what="partly filtered")


def _check_grid(new, max_blocks):
    rng = np.random.default_rng(13)
    sizes = rng.choice(np.array([0, 1, 1, 2, 3]), 70001)
    sizes[1000] = 200; sizes[69999] = 65
    off, h = random_batch(0, seed=14, sizes=sizes)
    check_against_restatement(new, off, h, "ISF", max_blocks=max_blocks, what="70 001 units, max_blocks %d" % max_blocks)
    check_against_restatement(new, off, h, "A", max_blocks=max_blocks, what="70 001 units, max_blocks %d" % max_blocks)


def check_grid_one_block(new):
    _check_grid(new, 1)


def check_grid_two_blocks(new):
    _check_grid(new, 2)


def check_grid_default(new):
    _check_grid(new, 0)


def check_state(new):
    """two sweeps add up; a clear between sweeps; add_counts of another object's counts"""
    a = random_batch(3000, seed=21); b = random_batch(777, seed=22)
    wa, _, _ = tally(*a, "ISR"); wb, _, _ = tally(*b, "ISR")
    f = new("ISR", 2); g = new("ISR", 0)
    try:
        f.add_hits(*a); f.add_hits(*b)
        assert_same(f.counts(), wa + wb, "ISR", "two sweeps")
        assert f.stat()["sweeps"] == 2 and f.stat()["mask"] == mask_of("ISR")
        f.clear()
        assert not f.counts().any() and f.stat()["sweeps"] == 0
        f.add_hits(*b)
        assert_same(f.counts(), wb, "ISR", "after clear")
        g.add_hits(*a)
        f.add_counts(g.counts())
        assert_same(f.counts(), wa + wb, "ISR", "add_counts")
        bad = np.zeros(32, dtype=np.uint64); bad[31] = 1
        try:
            f.add_counts(bad)
        except Exception as e:
            assert "-1" in str(e)                                    # QM_E_ARG
        else:
            raise AssertionError("counts[31] != 0 was accepted")
    finally:
        f.close(); g.close()


def check_no_hits(new):
    for n in (1, 64, 300):
        off = np.zeros(n + 1, dtype=np.int64)
        for hits in (None, np.zeros(0, dtype=HIT_DTYPE)):
            ew, eo, et = check_against_restatement(new, off, hits, "IU", what="%d units without hits" % n)
            assert int(ew[W_UNITS]) == n == int(ew[W_UNMAPPED]) and int(ew[:24].sum()) == 0 and not eo.any() and et.size == 0


CHECKS = {f.__name__[6:]: f for f in (check_sizes, check_wave_boundaries, check_code_edges, check_masks, check_keep_patterns, check_partly_filtered,
                                      check_grid_one_block, check_grid_two_blocks, check_grid_default, check_state, check_no_hits)}


def eqc_batches():
    """(name, hit_offsets, hits) for the qm_eqc_add_lib checks: repeated tids, partly filtered units, long units"""
    off, h = random_batch(4097, seed=31)
    yield "4097 hits", off, h
    rng = np.random.default_rng(32)
    sizes = rng.choice(np.array([0, 1, 2, 3, 9, 70]), 600)
    off, h = random_batch(0, seed=33, sizes=sizes)
    h["tid"] = rng.integers(0, 6, h.size)                            # few transcripts: repeats inside a unit, few classes
    yield "600 units over 6 transcripts", off, h


# ---- inference; fn(counts) is the implementation under test

def _single(**kw):
    c = np.zeros(32, dtype=np.uint64)
    for k, v in kw.items():
        c[W_SINGLE + CODES.index(k)] = v
    return c


INFER_CASES = [("80/20", _single(ISF=80, ISR=20), "ISF"), ("20/80", _single(ISF=20, ISR=80), "ISR"), ("70/30", _single(ISF=70, ISR=30), "IU"),
               ("30/70", _single(ISF=30, ISR=70), "IU"), ("71/29", _single(ISF=71, ISR=29), "ISF"), ("29/71", _single(ISF=29, ISR=71), "ISR"),
               ("no pairs", _single(), ""), ("orphans only", _single(LF=10, RR=10), ""),
               ("outward", _single(OSF=9, OSR=1, ISF=5, ISR=4), "OSF"), ("same strand", _single(MSF=1, MSR=9, ISF=5, ISR=4), "MSR"),
               ("tie I/O", _single(ISF=5, ISR=5, OSF=10), "IU"), ("tie O/M", _single(OSF=3, MSR=3), "OSF"),
               ("single-end", _single(SF=10, SR=10), "U"), ("single-end forward", _single(SF=8, SR=2), "SF"), ("single-end reverse", _single(SR=1), "SR"),
               ("large", _single(ISF=2 ** 59 - 1, ISR=2 ** 59 - 1), "IU"), ("large forward", _single(ISF=2 ** 59 - 1), "ISF")]


def check_infer(fn):
    for name, c, exp in INFER_CASES:
        assert infer(c) == exp, name
        assert fn(c) == exp, name
    rng = np.random.default_rng(41)
    for _ in range(200):
        c = np.zeros(32, dtype=np.uint64)
        c[W_SINGLE:W_SINGLE + 12] = rng.integers(0, 50, 12) * rng.integers(0, 2, 12)
        assert fn(c) == infer(c), c.tolist()
