"""Stage A over many trips per wavefront on the HIP path (libqmap_mi355.so through its C ABI), against the oracle.

Every stage-A kernel is a persistent grid: a wavefront maps work item gw, then gw + nw, gw + 2 nw, ...; between trips it carries the
LDS-DMA pipeline's two alternating buffers, the slab words that "stay zero", duo_prepare's registers of the pair ahead, the open chunk
of the list allocator and its scratch slot.  The families' batches (3 000 to 4 300 pairs) are smaller than the widest grid of a whole
device (65 536 wavefronts), so there every parity result of theirs is one prologue and one trip.  Here each leg maps
tile_cases.tile() of a base batch -- enough shuffled copies that every wavefront of the widest grid of the leg's first launch makes six
trips (tile_cases.copies_for, from the device's compute units) -- and holds the result bit for bit to the oracle's result of the base
batch gathered by the permutation (tile_cases.expected, which test_many_trips.py holds to the oracle).

After each call, those of -s too: the kernel it was meant for ran (check_headline, QM_STAT_LEAN_READS) and left some reads; its
first launch left and merged `copies` times what the untiled call on the same mapper did (deferral and merge are decided per read; the N-aware pass, decided per batch, may
then take the reads with N's out of what was left), and no launch was repeated.  With -s the trips of the list and alignment kernels
are reported, not asserted.  Measured on 256 compute units: 21 s for the module, 4.8 s for the slowest leg.  The grid knobs are read
once per process, so the smallest grid (one block per compute unit, no oversubscription: dozens of trips over four copies) runs in a
fresh child process: this file as a script.  No error path is provoked here."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [HERE, os.path.join(HERE, "emu"), os.path.dirname(HERE)]

import mapping_harness as mh
import tile_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def root(tmp_path_factory, lib_built, oracle_mod):
    yield tmp_path_factory.mktemp("many_trips_gpu")
    tc.forget_tiles()


@pytest.fixture(scope="module")
def num_cu(lib_built):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def mapper_of(leg, idx):
    if leg.mapper == "general":
        return mh.gpu_mapper(idx, debug=True)
    if leg.mapper == "wide":
        return mh.gpu_mapper(idx, debug=False, pair_kernel=False, wide_reads=True)
    return mh.headline(idx, leg.mapper, ph_compact=leg.compact)


def stats_of(mp):
    import rapmap_amd as ra
    return {k: mp.stat(getattr(ra, "QM_STAT_" + k)) for k in ("LEAN_READS", "LEAN_DEFERRED", "PAIR_KERNEL_PAIRS", "PAIRS_MERGED", "RELAUNCHES", "N_PASS_READS")}


def one_call(mp, leg, variant, opts, a, want, what, copies=1, base_stats=None):
    """one call of the leg's mapper over the packed reads `a`, held to `want` (the oracle's result, or tile_cases.expected of it) and,
    given the statistics of the untiled call on the same mapper, to `copies` times what that call left and merged -> the statistics"""
    n = len(a[1]) - 1
    got = mp.map_reads(*a, opts=opts) if leg.single else mp.map_pairs(*a, opts=opts)
    mh.check(want, got, what, ints=mp.intervals(n) if leg.ints and not mh.is_sel(variant) else None)
    st = stats_of(mp)
    reads = n if leg.single else 2 * n
    left = lambda s: s["LEAN_DEFERRED"] + s["N_PASS_READS"]
    if leg.mapper == "general":
        assert st["LEAN_READS"] == -1, (what, st)
    else:
        # also with -s: qm_lean_kernel (its collector edition) was the first launch over every read -- run_stage_a reports the reads of
        # SK_LEAN_SEL too -- and left some of them; a plan that fell back to the general collector reports -1 and leaves none
        assert st["LEAN_READS"] == reads, "%s: qm_lean_kernel / the pair kernel did not run: %r" % (what, st)
        assert 0 < left(st) < reads, (what, st)
        if leg.single:
            assert st["PAIR_KERNEL_PAIRS"] == -1, (what, st)
        elif not mh.is_sel(variant):
            # (the reads with N's are all that the ends family's batch leaves, and the N-aware pass of a tiled call maps every one of them)
            mh.check_headline(mp, leg.mapper if leg.mapper == "pair" else "lean", n, expect_deferred=st["N_PASS_READS"] == 0, fuzzy=variant.startswith("fuzzy"))
    if base_stats is not None:
        # what the first launch left is decided per read; whether the N-aware pass then takes the reads with N's out of it is decided per
        # batch (QM_NPASS_MIN: 2 048 reads with an odd character, which the tiled batch has and the base batch has not)
        assert left(st) == copies * left(base_stats), (what, copies, st, base_stats)
        if (st["N_PASS_READS"] > 0) == (base_stats["N_PASS_READS"] > 0):
            assert st["LEAN_DEFERRED"] == copies * base_stats["LEAN_DEFERRED"], (what, copies, st, base_stats)
        if leg.mapper == "pair" and not mh.is_sel(variant):
            assert st["PAIRS_MERGED"] == copies * base_stats["PAIRS_MERGED"], (what, copies, st, base_stats)
        if leg.npass:
            assert st["N_PASS_READS"] == copies * base_stats["N_PASS_READS"] > 0, (what, copies, st, base_stats)
    # the list and interval buffers are sized per read plus a chunk per wavefront of the grid, twice: the same lists per read, `copies`
    # times over, fit as the untiled call's did
    assert st["RELAUNCHES"] == (0 if base_stats is None else base_stats["RELAUNCHES"]) == 0, (what, st, base_stats)
    return st


def run_leg(leg, root, oracle_mod, num_cu):
    with mapper_of(leg, tc.base(leg.fam, root, oracle_mod, leg.k, leg.L, leg.image, leg.variants[0], single=leg.single).idx) as (qi, mp):
        assert qi.perfect_hash == (leg.image == "ph"), (qi.perfect_hash, leg.image)
        for variant in leg.variants:
            ints = leg.ints and not mh.is_sel(variant)
            b = tc.base(leg.fam, root, oracle_mod, leg.k, leg.L, leg.image, variant, single=leg.single, ints=ints)
            opts = mh.lib_opts(variant, oracle_mod)
            t0 = time.perf_counter()
            st0 = one_call(mp, leg, variant, opts, b.a, b.res, "untiled, " + b.what)
            copies, nw = tc.leg_copies(leg, variant, b.n, num_cu)
            note = ""
            if leg.npass:
                # the queue of the N-aware pass: what it mapped and what it left; its grid has no oversubscription, two reads of the queue per trip
                queue, nwq = st0["N_PASS_READS"] + st0["LEAN_DEFERRED"], tc.widest_waves("lean_nq", num_cu)
                assert st0["N_PASS_READS"] > 0 and queue > 0, st0
                copies = max(copies, -(-2 * tc.TRIPS * nwq // queue))
                trips_q = tc.trips_per_wave("lean_nq", copies * queue, False, nwq)
                assert trips_q[0] >= tc.TRIPS, (copies, queue, nwq, trips_q)
                note = "; the N-aware pass: %d reads of the queue over %d wavefronts, %d to %d trips" % ((copies * queue, nwq) + trips_q)
            units = copies * b.n
            assert units < tc.MAX_UNITS, "%s: %d copies of %d units are %d, not below %d (QM_HOST_CHUNK's default): %d compute units are too many for one launch" % (
                leg.id, copies, b.n, units, tc.MAX_UNITS, num_cu)
            trips = tc.trips_per_wave(leg.kernel, units, leg.paired, nw, leg.wide)
            assert trips[0] >= tc.TRIPS, (leg.id, variant, copies, units, nw, trips)
            a, want, perm = tc.tiled(b, copies, tc.SEED, ints=ints)
            t1 = time.perf_counter()
            one_call(mp, leg, variant, opts, a, want, "%d copies, %s" % (copies, b.what), copies, st0)
            if mh.is_sel(variant):                               # reported, no condition: the kernels of -s behind stage A
                import rapmap_amd as ra
                ksw = mp.stat(ra.QM_STAT_KSW2_ALIGNMENTS)
                lw, rows, aw, at = tc.sel_trips(units * (2 if leg.paired else 1), ksw, num_cu, int(max(np.diff(o).max() for o in a[1::2])))
                note += "; -s: list kernel %d wavefronts, %d reads in a row each; %d ksw2 alignments in %d chunk(s) over %d wavefronts, at most %d trip(s)" % (
                    lw, rows, ksw, 4 if units >= 4 * 65536 else 1, aw, at)
            print("%s %s: %d CUs, %d wavefronts, %d copies of %d = %d units, %d to %d trips per wavefront%s; untiled call and tiling %.2f s, tiled call and checks %.2f s"
                  % (leg.id, variant, num_cu, nw, copies, b.n, units, trips[0], trips[1], note, t1 - t0, time.perf_counter() - t1))


@pytest.mark.parametrize("leg", tc.LEGS, ids=lambda l: l.id)
def test_leg(root, oracle_mod, num_cu, leg, monkeypatch):
    """one mapper; per option set the untiled call and the tiled one, six trips and more per wavefront of the widest grid"""
    if leg.npass:
        monkeypatch.setenv("QM_NPASS_MIN", "1")
    run_leg(leg, root, oracle_mod, num_cu)


def test_smallest_grid(root, oracle_mod, num_cu, tmp_path):
    """QM_BLOCKS_PER_CU=1 QM_GRID_OVERSUB=1 QM_DUO_OVERSUB=1 in a fresh process: four copies of legs 1, 2 (paired, and the odd single-end count whose
    last trip holds one read), 3, 5 and 8 over a grid of one block per compute unit, held to the expectations made here"""
    arrays, jobs = {}, []
    for leg in (l for l in tc.LEGS if l.small):
        for variant in leg.variants:
            b = tc.base(leg.fam, root, oracle_mod, leg.k, leg.L, leg.image, variant, single=leg.single)
            a, want, perm = tc.tiled(b, tc.SMALL_COPIES, tc.SEED + 1)
            tag = "%s.%s" % (leg.id, variant)
            nw = tc.widest_waves(leg.kernel, num_cu, smallest=True)
            trips = tc.trips_per_wave(leg.kernel, tc.SMALL_COPIES * b.n, leg.paired, nw)
            assert trips[0] >= tc.TRIPS, (tag, nw, trips)
            print("%s: smallest grid%s, %d wavefronts, %d copies of %d units, %d to %d trips per wavefront" % ((tag, " -s" if mh.is_sel(variant) else "", nw, tc.SMALL_COPIES, b.n) + trips))
            jobs.append("%s\t%s" % (tag, b.idx))
            for j, x in zip(("q1", "o1", "q2", "o2"), a):              # (single-end: q1, o1 alone)
                arrays["%s.%s" % (tag, j)] = x
            for j, x in zip(("b_q1", "b_o1", "b_q2", "b_o2"), b.a):
                arrays["%s.%s" % (tag, j)] = x
            arrays[tag + ".offsets"], arrays[tag + ".hits"] = want.hit_offsets, np.frombuffer(want.hits.tobytes(), dtype=np.uint8)
            arrays[tag + ".counters"] = np.array([want.counters[k] for k in tc.COUNTERS], dtype=np.int64)
    f = str(tmp_path / "want.npz")
    np.savez(f, jobs=np.array(jobs), **arrays)
    e = {k: v for k, v in os.environ.items() if k not in tc.GRID_KNOBS}
    e.update(tc.SMALLEST_GRID)
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, os.path.abspath(__file__), f], env=e, capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:])
    print("the child process: %.2f s" % (time.perf_counter() - t0))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "many trips ok" in p.stdout.splitlines()[-1]


def _child(path):
    """the jobs of `path` under this process's grid knobs: per job the untiled call, then the four copies, against the parent's expectations"""
    import torch
    torch.cuda.init()                                            # (torch's HIP runtime opens the device before the library's: conftest.lib_built)
    import types
    from oracle import oracle
    from rapmap_amd.api import HIT_DTYPE
    assert all(os.environ.get(k) == v for k, v in tc.SMALLEST_GRID.items()), "the grid knobs are not set"
    z = np.load(path)
    legs = {l.id: l for l in tc.LEGS}
    open_leg, cm, mp = None, None, None
    try:
        for job in z["jobs"].tolist():
            tag, idx = job.split("\t")
            leg_id, variant = tag.split(".", 1)
            leg = legs[leg_id]
            if open_leg != leg_id:
                if cm is not None:
                    cm.__exit__(None, None, None)
                cm = mapper_of(leg, idx)
                qi, mp = cm.__enter__()
                open_leg = leg_id
            want = types.SimpleNamespace(hit_offsets=z[tag + ".offsets"], hits=z[tag + ".hits"].view(HIT_DTYPE),
                                         counters=dict(zip(tc.COUNTERS, [int(x) for x in z[tag + ".counters"]])))
            opts = mh.lib_opts(variant, oracle)
            names = ("q1", "o1") if leg.single else ("q1", "o1", "q2", "o2")
            base_a = tuple(z["%s.b_%s" % (tag, j)] for j in names)
            got0 = mp.map_reads(*base_a, opts=opts) if leg.single else mp.map_pairs(*base_a, opts=opts)
            st0 = stats_of(mp)
            assert st0["RELAUNCHES"] == 0 and st0["LEAN_READS"] == (len(base_a[1]) - 1) * (1 if leg.single else 2), (tag, st0)
            assert got0.counters == {k: v // tc.SMALL_COPIES for k, v in want.counters.items()}, (tag, got0.counters, want.counters)
            one_call(mp, leg, variant, opts, tuple(z["%s.%s" % (tag, j)] for j in names), want, "smallest grid, " + tag, tc.SMALL_COPIES, st0)
            print("smallest grid, %s: ok" % tag)
    finally:
        if cm is not None:
            cm.__exit__(None, None, None)
    print("many trips ok")


if __name__ == "__main__":
    _child(sys.argv[1])
