"""A family's batch, tiled and shuffled: what test_many_trips.py (the oracle and the lane emulation) and test_many_trips_gpu.py (the HIP
path) share.  Every stage-A kernel is a persistent grid whose wavefront gw maps work item gw, gw + nw, gw + 2 nw, ...; the batches of the
families (3 000 to 4 300 pairs) are smaller than the widest grid of a whole device (65 536 wavefronts), so no wavefront of theirs makes
a second trip there.  The reads of a batch are mapped independently of each other, so the oracle's result for `copies` shuffled copies
of a batch is its result of the base batch gathered by the permutation: tile() makes the batch, expected() the result, and the oracle
maps the base batch alone (base(), cached for the process).  test_many_trips.py holds that claim to the oracle itself.

No test functions here.  The asserts of this module are not rewritten by pytest, so each carries its values in its message."""
import os
import types

import numpy as np

import mapping_harness as mh
from util import pack

GRID_KNOBS = ("QM_BLOCKS_PER_CU", "QM_GRID_OVERSUB", "QM_GRID_OVERSUB_PH", "QM_DUO_OVERSUB")
SMALLEST_GRID = {"QM_BLOCKS_PER_CU": "1", "QM_GRID_OVERSUB": "1", "QM_DUO_OVERSUB": "1"}
TRIPS = 6              # the pipeline looks two trips ahead and alternates two buffers: six trips show each buffer three times in steady state
MAX_UNITS = 1 << 20    # QM_HOST_CHUNK's default: a host batch below it is one launch
COUNTERS = ("peHits", "seHits", "totHits", "numReads", "tooManyHits", "mappedUnits")


# ---- tiling

def _gather(off, rec, perm):
    """the records of units perm[0], perm[1], ... of (off, rec) in a row -> (offsets, records); no loop over units"""
    off = np.asarray(off, dtype=np.int64)
    cnt = np.diff(off)[perm]
    new = np.zeros(perm.size + 1, dtype=np.int64)
    np.cumsum(cnt, out=new[1:])
    src = np.repeat(off[:-1][perm] - new[:-1], cnt) + np.arange(new[-1], dtype=np.int64)
    return new, rec[src]


def permutation(n, copies, seed):
    """np.arange(copies * n) % n under the permutation of default_rng(seed): base unit perm[i] stands at place i"""
    return np.random.default_rng(seed).permutation(np.arange(copies * n, dtype=np.int64) % n)


def tile(a, copies, seed):
    """a: packed reads, (q1, o1, q2, o2) or (q, o) -> (the packed reads of copies x n units, perm).  Both mates of a pair move together."""
    n = len(a[1]) - 1
    perm = permutation(n, copies, seed)
    out = []
    for q, o in zip(a[0::2], a[1::2]):
        assert len(o) - 1 == n, (len(o) - 1, n)
        no, nq = _gather(o, np.asarray(q), perm)
        out += [nq, no]
    return tuple(out), perm


def expected(res, perm, copies, ints=False):
    """the oracle's result of tile(a, copies, seed) from its result `res` of a: the hit records of unit i are those of base unit perm[i]
    (qm_hit names no unit: copied as they are), every counter -- all six are sums over units -- is `copies` times the base's.  ints: the
    SA-interval records too (the two reads of a pair share one offset, the `list` column says whose a record is, so they move with their
    pair); mapping_harness.check() and check_intervals() take the result as they take the oracle's"""
    assert perm.size == copies * (len(res.hit_offsets) - 1), (perm.size, copies, len(res.hit_offsets) - 1)
    e = types.SimpleNamespace()
    e.hit_offsets, e.hits = _gather(res.hit_offsets, res.hits, perm)
    assert tuple(res.counters) == COUNTERS, res.counters
    e.counters = {k: copies * v for k, v in res.counters.items()}
    if ints:
        e.ints_offsets, e.ints = _gather(res.ints_offsets, res.ints, perm)
    return e


# ---- the grids.  Every factor is a literal with the line of rapmap_amd/csrc/qm_grid.h it restates; nothing is imported from the library.

def knobs_unset():
    bad = {k: os.environ[k] for k in GRID_KNOBS if k in os.environ}
    assert not bad, "a grid knob is set in this process: %r" % bad


def widest_waves(kernel, num_cu, sel=False, compact=False, smallest=False):
    """the wavefronts of the widest grid the launch layer gives a kernel on num_cu compute units: resident blocks per CU (at most 8) x
    oversubscription x 4 waves per block.  kernel: "pair", "lean", "lean_nq" (the N-aware pass), "general".  smallest: under
    SMALLEST_GRID (one resident block per CU, G = 1, QM_DUO_OVERSUB = 1; the compact image's factor falls back to G)"""
    if smallest:
        return num_cu * 1 * 1 * 4
    over = {"pair": 12 if compact else 8,                          # qm_duo_kernel: PH ? P : 2 G      (G = 4, P = 12)
            "lean": 12 if compact else 4 if sel else 8,            # qm_lean_kernel: PH ? P : SEL ? G : 2 G
            "lean_nq": 1,                                          # qm_lean_kernel: NQ ? 1
            "general": 12 if compact else 4}[kernel]               # qm_read_kernel: F & QM_F_PH ? P : G (map_grid)
    return num_cu * 8 * over * 4


def work_items(kernel, units, paired, wide=False):
    """trips the whole grid makes over `units` units: qm_grid.h's pair_iters / lean_iters, one read per trip for the general kernel"""
    reads = 2 * units if paired else units
    if kernel == "pair":
        return reads >> 1
    if kernel in ("lean", "lean_nq"):
        return reads if wide else (reads + 1) >> 1
    return reads


def trips_per_wave(kernel, units, paired, nw, wide=False):
    """(fewest, most) trips of a wavefront: wave gw takes items gw, gw + nw, ..."""
    w = work_items(kernel, units, paired, wide)
    return w // nw, (w + nw - 1) // nw


def copies_for(kernel, n_base, num_cu, trips=TRIPS, paired=True, wide=False, sel=False, compact=False):
    """the smallest `copies` for which every wavefront of the widest grid makes at least `trips` trips over copies x n_base units"""
    knobs_unset()
    nw = widest_waves(kernel, num_cu, sel=sel, compact=compact)
    need = trips * nw                                          # the last wave, nw - 1, makes `trips` trips once there are trips x nw items
    c = max(1, need * 1000 // work_items(kernel, 1000 * n_base, paired, wide) - 1)
    while work_items(kernel, c * n_base, paired, wide) < need:
        c += 1
    while c > 1 and work_items(kernel, (c - 1) * n_base, paired, wide) >= need:
        c -= 1
    return c


def unit_stride(kernel, nw, paired, wide=False):
    """by how many units the successive items of one wavefront lie apart (nw is even): the pair kernel a pair per trip, qm_lean_kernel two
    reads (a pair; single-end: two units), its wide edition and the general kernel one read (half a pair)"""
    if kernel == "pair":
        return nw
    if kernel in ("lean", "lean_nq") and not wide:
        return nw if paired else 2 * nw
    return nw // 2 if paired else nw


# ---- what stands behind what

def kinds(a, res, k, per_mate=False):
    """per base unit, from the reads and the oracle's result alone (res: default options, with the SA-interval records where the call is
    paired): dirty -- a mate holds a character outside ACGT (an N ...); short -- a mate shorter than k, or empty; nohit; many -- an SA
    interval of 64 suffixes or more (a mate's hits before they are reduced to one per transcript: the final records name a transcript
    once, and no family has a read on 64 transcripts); longest -- a mate of more than 100 characters; clean_mapped.
    per_mate (paired, with interval records): [the kinds of mate 1, of mate 2], for the kernels that give a wavefront one READ per trip
    -- the hit-based kinds then come from the read's own interval records (column `list`: 0 / 1 mate 1, 2 / 3 mate 2): nohit -- none,
    many -- one of 64 suffixes or more"""
    n = len(a[1]) - 1
    odd = np.ones(256, bool)
    odd[list(b"ACGT")] = False
    mates = []
    for q, o in zip(a[0::2], a[1::2]):
        o = np.asarray(o, dtype=np.int64)
        c = np.concatenate([[0], np.cumsum(odd[np.asarray(q)])])
        mates.append({"dirty": (c[o[1:]] - c[o[:-1]]) > 0, "short": np.diff(o) < k, "longest": np.diff(o) > 100})
    if per_mate:
        assert len(mates) == 2 and hasattr(res, "ints"), "per-read kinds need a paired result with its interval records"
        unit = np.repeat(np.arange(n), np.diff(res.ints_offsets))
        mate = res.ints[:, 5] >> 1
        assert ((mate == 0) | (mate == 1)).all(), "interval records with a list other than 0 .. 3"
        wide = (res.ints[:, 1].astype(np.int64) - res.ints[:, 0]) >= 64
        for m, kd in enumerate(mates):
            has = np.zeros(n, bool); has[unit[mate == m]] = True
            kd["many"] = np.zeros(n, bool); kd["many"][unit[(mate == m) & wide]] = True
            kd["nohit"], kd["clean_mapped"] = ~has, ~kd["dirty"] & has
        return mates
    kd = {x: np.logical_or.reduce([m[x] for m in mates]) for x in ("dirty", "short", "longest")}
    nh = np.diff(np.asarray(res.hit_offsets))
    kd["many"] = np.zeros(n, bool)
    if hasattr(res, "ints"):
        wide = (res.ints[:, 1].astype(np.int64) - res.ints[:, 0]) >= 64
        kd["many"][np.repeat(np.arange(n), np.diff(res.ints_offsets))[wide]] = True
    kd["nohit"], kd["clean_mapped"] = nh == 0, ~kd["dirty"] & (nh > 0)
    return kd


COMBOS = (("dirty", "clean_mapped"), ("many", "nohit"), ("longest", "short"))
AT_LEAST = 100


def per_read(kernel, paired, wide=False):
    """the kernel gives a wavefront one read of a pair per trip: the general kernel and the wide lean edition.  Its grid has an even
    number of wavefronts, so a wavefront meets the same mate every trip, a pair further on each time"""
    return paired and (kernel == "general" or wide)


def neighbours(perm, stride, kd, combos=COMBOS):
    """how often units (i, i + stride) of the tiled batch -- successive items of one wavefront -- are of kinds (first, then).  kd: kinds()
    of the base batch; its per_mate form for a per_read() kernel: mate 1 then mate 1, plus mate 2 then mate 2"""
    out = {}
    for first, then in combos:
        out[(first, then)] = sum(int((d[first][perm[:-stride]] & d[then][perm[stride:]]).sum()) for d in (kd if isinstance(kd, list) else [kd])) if stride < perm.size else 0
    return out


# ---- the base batches: a family's reads with more of the kinds that are rare in it, made from the reads alone

BOOST = 250      # pairs of each kind added behind a family's: with them every combination of COMBOS reaches AT_LEAST in the general kernel's
                 # batch too, the smallest (98 304 pairs on 256 CUs): 81 920 neighbours x (250 / 5 000)^2 = 205


def _boost(r1, r2, k, seed, each=BOOST):
    """behind (r1, r2), `each` pairs of: random characters (no hit); one mate cut to k - 1, 5 or 0 characters; an N somewhere in one mate;
    mate 1 made 120 characters long with random characters behind it (more than 100, still the narrow kernels' reads)"""
    rng = np.random.default_rng(seed)
    n = len(r1)
    r1, r2 = list(r1), list(r2)
    pick = lambda: int(rng.integers(0, n))
    for j in range(each):
        L = len(r1[pick()]) or 50
        r1.append(mh.ACGT[rng.integers(0, 4, L)].tobytes()); r2.append(mh.ACGT[rng.integers(0, 4, L)].tobytes())
    for j in range(each):
        i, cut = pick(), (k - 1, 5, 0)[j % 3]
        r1.append(r1[i][:cut] if j % 2 == 0 else r1[i]); r2.append(r2[i][:cut] if j % 2 == 1 else r2[i])
    for j in range(each):
        i = pick()
        m = bytearray(r2[i] if j % 2 else r1[i])
        if m:
            m[int(rng.integers(0, len(m)))] = ord("N")
        r1.append(r1[i] if j % 2 else bytes(m)); r2.append(bytes(m) if j % 2 else r2[i])
    for j in range(each):
        i = pick()
        r1.append((r1[i] + mh.ACGT[rng.integers(0, 4, 120)].tobytes())[:max(120, len(r1[i]))]); r2.append(r2[i])
    return r1, r2


def _family(name):
    import ends_cases
    import kmer_cases as kc
    import repeat_cases

    def of(mod):
        return lambda k, L: (mod.reads_for(k, L)["r1"], mod.reads_for(k, L)["r2"])
    return {"golden": types.SimpleNamespace(index_for=kc.index_for, reads=lambda k, L: (kc.golden_reads()[1], kc.golden_reads()[3])),
            "repeats": types.SimpleNamespace(index_for=repeat_cases.index_for, reads=of(repeat_cases)),
            "ends": types.SimpleNamespace(index_for=ends_cases.index_for, reads=of(ends_cases))}[name]


def reads_of(name, root, oracle_mod, k, L, limit=None):
    """(reads1, reads2) of a base batch: a family's pairs and _boost's behind them; limit: the first `limit` pairs of the family alone.
    The golden reads at k below 31 hold a handful of pairs with an interval of 64 suffixes (kinds(): many): BOOST more copies of those,
    found by the oracle under default options, go behind the others"""
    def make():
        r1, r2 = _family(name).reads(k, L)
        if limit:
            return list(r1[:limit]), list(r2[:limit])
        r1, r2 = _boost(r1, r2, k, 1000 * k + L)
        if name == "golden" and k < 31:
            a = pack(r1) + pack(r2)
            res = mh.oracle_of(_family(name).index_for(root, k, "dense"))[1].map_pairs(*a, opts=mh.oracle_opts("default", oracle_mod), nthreads=8, want_ints=True)
            many = np.nonzero(kinds(a, res, k)["many"])[0]
            assert many.size, "no golden pair with an interval of 64 suffixes at k=%d" % k
            r1 += [r1[many[j % many.size]] for j in range(BOOST)]; r2 += [r2[many[j % many.size]] for j in range(BOOST)]
        return r1, r2
    return mh.once(("tile_reads", name, k, L, limit), make)


def base(name, root, oracle_mod, k, L, image, variant, single=False, ints=False, limit=None):
    """the oracle's result of a base batch, computed once and shared (never changed), as mapping_harness.ref() gives it:
    -> .idx, .a (the packed reads), .n (units), .res, .what, .k, .key (of the reads)"""
    idx = _family(name).index_for(root, k, "dense" if image == "dense" else "ph")
    r1, r2 = reads_of(name, root, oracle_mod, k, L, limit)
    key = (name, k, L, limit, single)
    a = mh.once(("tile_packed",) + key, lambda: pack(mh.odd_single(r1, r2)) if single else pack(r1) + pack(r2))
    what = "%s k=%d L=%d %s %s%s" % (name, k, L, image, variant, ", single-end" if single else "")

    def make():
        orc, oopts = mh.oracle_of(idx)[1], mh.oracle_opts(variant, oracle_mod)
        return orc.map_single(*a, opts=oopts, nthreads=8) if single else orc.map_pairs(*a, opts=oopts, nthreads=8, want_ints=ints)
    res = mh.once(("tile_base", idx, variant, ints) + key, make)
    return types.SimpleNamespace(idx=idx, a=a, n=len(a[1]) - 1, res=res, what=what, k=k, key=key)


def kinds_of(name, root, oracle_mod, k, L, single=False, per_mate=False):
    """kinds() of a base batch: a fact of the data, asked of the oracle under default options on the dense index"""
    b = base(name, root, oracle_mod, k, L, "dense", "default", single=single, ints=not single)
    return mh.once(("tile_kinds", per_mate) + b.key, lambda: kinds(b.a, b.res, k, per_mate=per_mate))


_tiles = {}


def tiled(b, copies, seed, ints=False):
    """(the packed reads of tile(b.a, copies, seed), expected(b.res, ...), perm); the reads are built once per base batch, copies and
    seed and kept until forget_tiles()"""
    key = b.key + (copies, seed)
    if key not in _tiles:
        _tiles[key] = tile(b.a, copies, seed)
    a, perm = _tiles[key]
    return a, expected(b.res, perm, copies, ints=ints), perm


def forget_tiles():
    """the tiled batches are a few hundred MB: a module drops them when it is done"""
    _tiles.clear()


# ---- the legs of test_many_trips_gpu.py, the smallest set that reaches every loop.  mapper: "pair" / "lean" -- mapping_harness.headline;
# "wide" -- headline's lean mapper with the wide extension table; "general" -- debug=True, which keeps the SA-interval records.  kernel: the
# first launch of stage A, whose grid decides the copies (with -s the lean kernel's collector edition stands in for the pair kernel).

def _leg(id, fam, mapper, kernel, variants, k=31, L=100, image="dense", single=False, wide=False, compact=False, npass=False, small=False):
    return types.SimpleNamespace(id=id, fam=fam, mapper=mapper, kernel=kernel, variants=variants, k=k, L=L, image=image, single=single, wide=wide,
                                 compact=compact, npass=npass, small=small, paired=not single, ints=mapper == "general")


LEGS = [
    _leg("1_golden_pair", "golden", "pair", "pair", ("default", "noStrictCheck", "z0.9"), small=True),
    _leg("2_golden_lean", "golden", "lean", "lean", ("default", "fuzzy"), small=True),
    _leg("2_golden_lean_single", "golden", "lean", "lean", ("default", "fuzzy"), single=True, small=True),
    _leg("3_golden_sel", "golden", "pair", "lean", ("selAln", "mimicBT2"), small=True),
    _leg("4_golden_n_pass", "golden", "lean", "lean", ("default",), npass=True),
    _leg("5_repeats_pair", "repeats", "pair", "pair", ("default", "maxInterval50"), small=True),
    _leg("5_repeats_lean", "repeats", "lean", "lean", ("default", "maxInterval50"), small=True),
    _leg("6_ends_100", "ends", "pair", "pair", ("default", "noDovetail")),
    _leg("6_ends_64", "ends", "pair", "pair", ("default", "noDovetail"), L=64),
    _leg("7_repeats_wide_150", "repeats", "wide", "lean", ("default", "selAln"), L=150, wide=True),
    _leg("7_ends_wide_250", "ends", "wide", "lean", ("default", "selAln"), L=250, wide=True),
    _leg("8_golden_compact", "golden", "lean", "lean", ("default",), image="ph", compact=True, small=True),
    _leg("9_golden_general", "golden", "general", "general", ("default", "noSensitive", "fuzzy")),
    _leg("9_repeats_general_ns4", "repeats", "general", "general", ("default",), L=250),
    _leg("10_golden_k15_pair", "golden", "pair", "pair", ("default",), k=15),
    _leg("10_golden_k15_lean", "golden", "lean", "lean", ("default",), k=15),
    _leg("10_golden_k21_pair", "golden", "pair", "pair", ("default",), k=21),
    _leg("10_golden_k21_lean", "golden", "lean", "lean", ("default",), k=21),
]
SMALL_COPIES = 4      # the smallest-grid leg: four copies of the legs marked small
SEED = 2024


def leg_copies(leg, variant, n_base, num_cu):
    """(copies, wavefronts of the widest grid of the leg's first launch) on num_cu compute units"""
    sel = mh.is_sel(variant)
    nw = widest_waves(leg.kernel, num_cu, sel=sel, compact=leg.compact)
    return copies_for(leg.kernel, n_base, num_cu, paired=leg.paired, wide=leg.wide, sel=sel, compact=leg.compact), nw


def sel_trips(reads, alignments, num_cu, max_len):
    """-s behind stage A, reported and no condition (qm_kernels.hip): the list kernel qm_h2m_pack_kernel gives every wavefront one
    contiguous range of reads -- at most 2 resident blocks per CU x G = 4 -- and the register edition of the alignment kernel (the
    default band) strides over the ksw2 alignments eight to a wavefront and trip, 8 blocks per CU x G (reads beyond 192 characters: 7).
    A batch below 4 x 65 536 units is one chunk of plan -> ksw2 -> finish.  -> (list wavefronts, reads per list wavefront, alignment
    wavefronts, trips of an alignment wavefront at the most)"""
    lw = num_cu * 2 * 4 * 4                                        # qmk_h2m_pack: resident_per_cu fallback 2, grid_oversub()
    aw = num_cu * (8 if max_len <= 192 else 7) * 4 * 4             # qmk_sel_align_finish: num_cu * 8 * ao (or 7), ao = grid_oversub()
    return lw, -(-reads // lw), aw, -(-(-(-alignments // 8)) // aw)
