"""The positional bias model without a GPU: classes and bins, the observed sweep, the expected counts, the effective lengths and their
driver (rapmap_amd/csrc/qm_psb.inl, qm_psb_host.inl) under the lane emulation, and the pure host function (ratios) through the built
library and through the emulation's build of the same text.

The emulation (tests/emu/qm_emu_psb.cpp) runs one wavefront after the other and one lane after the other, every slab filled with
0xA5: it proves the LOGIC of the bodies -- psb_bin and its settling comparisons, categories, the tally, the closed form of the
expected counts against a term per position, the walk of qm_sqb.inl over this model's end biases, the order of every float sum, the
grid's cap -- and the driver's text, not the atomics; what contention does to them is the GPU tests' part (test_pos_bias_gpu.py).
Every comparison is exact."""
import numpy as np
import pytest

import gcb_cases as gc
import part_cases as pc
import psb_cases as ps
import sqb_cases as sq
from conftest import load_oracle
from util import pack


@pytest.fixture(scope="module")
def emu():
    import emu_psb
    emu_psb._lib()
    return emu_psb


@pytest.fixture(scope="module")
def world():
    w = gc.make_world(ps.crafted_seqs())
    for a in w.values():
        a.setflags(write=False)
    assert [int(x) for x in w["lens"]] == list(ps.LENS)
    return w


def _new(emu, w, **caps):
    return lambda max_len, max_blocks: emu.EmuPsb(w["off"], w["lens"], max_len, max_blocks, **caps)


def test_emulated_positions(emu, world):
    ps.check_positions(world, _new(emu, world))
    # by hand: L = 21 -- 20 x / 21: position 1 is bin 0 (20 / 21), position 2 bin 1 (40 / 21), position 20 bin 19; class bounds
    g = _new(emu, world)(1000, 0)
    lens = list(ps.LENS)
    try:
        got = g.position([lens.index(21)] * 3 + [lens.index(791), lens.index(792), lens.index(2433), lens.index(2434), lens.index(1)], [1, 2, 20, 790, 0, 2432, 1217, 0])
    finally:
        g.close()
    assert got.tolist() == [[0, 0], [0, 1], [0, 19], [0, 19], [1, 0], [3, 19], [4, 10], [0, 0]]


def test_emulated_bins_of_long_transcripts(emu):
    """psb_bin where 20 x leaves 32 bits: transcripts of up to 2^31 - 1 characters (the probe reads a length, no text), the bin edges
    and their neighbours against Python integers"""
    for L in (2 ** 31 - 1, 2 ** 31 - 2, 2 ** 30 + 1, 1 << 30, 3 * 5 * 7 * 11 * 13 * 17 * 19 * 23, 20 * 107374182, 4294967 * 499, 999999937):
        assert L < 2 ** 31
        xs = sorted({x for b in range(21) for x in (ps.edge(b, L) - 1, ps.edge(b, L), ps.edge(b, L) + 1, ps.edge(b, L) + 12345) if 0 <= x < L})
        g = emu.EmuPsb([0], [L])
        try:
            got = g.position([0] * len(xs), xs)
        finally:
            g.close()
        assert got[:, 1].tolist() == [ps.bin_of(v, L) for v in xs] and (got[:, 0] == 4).all() and got[:, 1].min() == 0 and got[:, 1].max() == 19


@pytest.mark.parametrize("check", sorted(ps.OBS_CHECKS))
def test_emulated_observed(emu, world, check):
    ps.OBS_CHECKS[check](world, _new(emu, world))


def test_emulated_grid_cap(emu):
    L = emu._lib()
    assert L.qe_psb_obs_grid(70001, 1) == 1 and L.qe_psb_obs_grid(70001, 2) == 2 and L.qe_psb_obs_grid(70001, 0) == 274 and L.qe_psb_obs_grid(10 ** 7, 0) == 2048
    assert L.qe_psb_exp_grid(23, 0) == 2 and L.qe_psb_exp_grid(23, 1) == 1 and L.qe_psb_exp_grid(10 ** 6, 0) == 2048
    assert L.qe_psb_tile_grid(10 ** 7, 0) == 1024 and L.qe_psb_tile_grid(5, 0) == 2 and L.qe_psb_tile_grid(5, 1) == 1


@pytest.mark.parametrize("shape", sorted(pc.SHAPES))
def test_emulated_host_arrays_in_parts(emu, world, shape):
    """qm_psb_add_hits' driver at MAX_UNITS units and MAX_ITEMS hits to a part: the same counts and counters as in one part and as the
    restatement; one fold per part"""
    off = pc.offsets_of(shape)
    hits = None
    if shape != "null":
        rng = np.random.default_rng(len(shape))
        _, hits = gc.build(world, rng.choice(np.array([gc.U, gc.U, gc.NP, gc.SS, gc.OOR, gc.OVH]), int(off[-1])), 1000, rng)
        assert hits.size == int(off[-1])
    small = _new(emu, world, max_units=pc.MAX_UNITS, max_hits=pc.MAX_ITEMS)
    whole = _new(emu, world, max_units=pc.ONE_PART, max_hits=pc.ONE_PART)
    c1, s1 = ps.fold_once(whole, off, hits)
    c, s = ps.fold_once(small, off, hits)
    eo, es = ps.classify(world, off, hits, 1000)
    ps.assert_same(c, s, eo, es, shape); ps.assert_same(c1, s1, eo, es, shape + ", one part")
    assert s["folds"] == len(pc.parts(off)) and s1["folds"] == min(len(off) - 1, 1)


def test_emulated_decreasing_offsets_leave_the_object_alone(emu, world):
    off, h = gc.random_batch(world, 300, 1000, seed=3)
    f = _new(emu, world, max_units=pc.MAX_UNITS, max_hits=pc.MAX_ITEMS)(1000, 0)
    try:
        f.add_hits(off, h)
        before = (f.counts(), f.stat())
        with pytest.raises(emu.ArgError):
            f.add_hits(pc.decreasing(), h)
        assert np.array_equal(f.counts(), before[0]) and f.stat() == before[1]
    finally:
        f.close()


@pytest.mark.parametrize("check", sorted(ps.EXPECT_CHECKS))
def test_emulated_expect(emu, world, check):
    ps.EXPECT_CHECKS[check](world, _new(emu, world))


@pytest.mark.parametrize("check", sorted(ps.EFF_CHECKS))
def test_emulated_eff_lens(emu, world, lib_built, check):
    if check == "ratio_one":
        import rapmap_amd as ra
        ps.check_eff_ratio_one(world, _new(emu, world), ra.eff_lens_from_counts)
    else:
        ps.EFF_CHECKS[check](world, _new(emu, world))


def test_ratios(emu, lib_built):
    import rapmap_amd as ra
    ps.check_ratios(ra.pos_bias_ratios)
    ps.check_ratios(emu.ratios)
    with pytest.raises(ValueError):
        ra.pos_bias_ratios(np.zeros(25, dtype=np.uint64), np.zeros(200, dtype=np.uint64))


def test_exports(lib_built):
    import rapmap_amd as ra
    assert ra.PSB_BINS == 200 and ra.PSB_STATS == ps.STATS and ra.PosBias.STATS[8:] == ("max_len", "folds", "last_fold_us", "last_expect_us", "last_efflen_us")
    for name in ("qm_psb_create", "qm_psb_destroy", "qm_psb_clear", "qm_psb_add", "qm_psb_add_hits", "qm_psb_add_counts", "qm_psb_fetch", "qm_psb_stat",
                 "qm_psb_expect", "qm_psb_eff_lens", "qm_psb_position", "qm_psb_ratios", "qm_stream_psb_fetch"):
        assert name in ra.ABI_SYMBOLS and getattr(ra.api.lib(), name)


def test_pos_bias_file_round_trip(tmp_path):
    import rapmap_amd as ra
    rng = np.random.default_rng(3)
    obs = rng.integers(0, 1 << 40, ps.SHAPE).astype(np.uint64); ex = rng.integers(0, 1 << 62, ps.SHAPE).astype(np.uint64); ex[1, 4, 19] = 2 ** 64 - 1
    ratio = np.exp2(rng.uniform(-2, 2, ps.SHAPE)); ratio[0, 3, :] = 1.0
    p = str(tmp_path / "q.sf.posBias.txt")
    ra.write_pos_bias(p, obs, ex, ratio)
    lines = open(p).read().split("\n")
    assert lines[0] == "end\tclass\tbin\tobs\texp\tratio" and len(lines) == 202 and lines[201] == "" and lines[66] == "0\t3\t5\t%d\t%d\t1" % (int(obs[0, 3, 5]), int(ex[0, 3, 5]))
    assert lines[200].startswith("1\t4\t19\t") and lines[200].split("\t")[5] == "%.17g" % ratio[1, 4, 19]
    o, e, r = ra.read_pos_bias(p)
    assert o.dtype == np.uint64 and np.array_equal(o, obs) and e.dtype == np.uint64 and np.array_equal(e, ex) and r.tobytes() == ratio.tobytes()
    open(p, "w").write("nonsense\n")
    with pytest.raises(ValueError):
        ra.read_pos_bias(p)


def _index_world(idx):
    import rapmap_amd as ra
    qi = ra.QuasiIndex(idx)
    text, off = qi.arrays()
    w = {"text": text, "off": off, "lens": np.asarray(qi.txp_lens, dtype=np.int64)}
    qi.close()
    return w


def test_emulated_synth_small(emu, synth_small, oracle_mod):
    """the oracle's hits of synth_small over the index's own transcripts; then that run's own histogram and weights through the expected
    counts, the ratios and the effective lengths"""
    import fld_cases as fc
    w = _index_world(synth_small["idx"])
    ix, orc = load_oracle(synth_small["idx"])
    q1, o1 = pack(synth_small["reads1"]); q2, o2 = pack(synth_small["reads2"])
    res = orc.map_pairs(q1, o1, q2, o2, nthreads=4)
    eo, es = ps.check_against_restatement(w, _new(emu, w), res.hit_offsets, res.hits, max_blocks=3, what="synth_small")
    assert es["units"] == 4234 and es["used"] >= 500, es
    counts, _ = fc.classify(res.hit_offsets, res.hits, 1000)
    T = w["lens"].size
    alpha = np.random.default_rng(5).random(T) * 50
    q, k = emu.weights(alpha, w["lens"], counts)
    assert np.array_equal(q, sq.weights(alpha, w["lens"], counts)[0]) and sq.weight_bound(q, w["lens"], counts) < 2 ** 63
    g = _new(emu, w)(1000, 0)
    try:
        ex = g.expect(counts, T, q)
        exp, total = ps.expect(w, counts, q)
        assert np.array_equal(ex, exp)
        ps.assert_two_ends(ex, total, "synth_small")
        R = emu.ratios(eo, ex)
        assert R.tobytes() == ps.ratios(eo, ex).tobytes() and (R != 1.0).any()
        e = g.eff_lens(counts, T, R)
        assert e.tobytes() == ps.eff_lens(w["lens"], counts, R).tobytes()
    finally:
        g.close()
    rs = orc.map_single(q1, o1, nthreads=4)
    eo, es = ps.check_against_restatement(w, _new(emu, w), rs.hit_offsets, rs.hits, what="single-end")
    assert es["used"] == es["same_strand"] == es["out_of_range"] == es["overhang"] == 0 and es["not_paired"] > 500 and not eo.any()


def _planted(emu, tmp_path, seed):
    """the steps of `quasimap --quant --quantFLD --quantPosBias` on fragments with a planted bias -> (err0, err1, what was seen)"""
    import rapmap_amd as ra
    from rapmap_amd import synth
    import eqc_cases as ec
    import fld_cases as fc
    import quant_cases as qc
    names, txps, theta = ps.planted_transcripts(seed)
    fa = str(tmp_path / ("planted%d.fa" % seed)); synth.write_fasta(fa, names, txps)
    idx = str(tmp_path / ("idx%d" % seed)); ra.build_index(fa, idx, threads=2)
    r1, r2, origin = ps.planted_fragments(txps, theta, seed=seed + 1)
    q1, o1 = pack(r1); q2, o2 = pack(r2)
    ix, orc = load_oracle(idx)
    res = orc.map_pairs(q1, o1, q2, o2, nthreads=4)
    off, hits = res.hit_offsets, res.hits
    T = len(txps)
    mapped = np.diff(off) > 0
    truth = np.bincount(origin[mapped], minlength=T).astype(np.float64)
    w = _index_world(idx)
    assert [int(x) for x in w["lens"]] == [t.size for t in txps]
    counts, fst = fc.classify(off, hits, 1000)
    graph = qc.Graph(*ec.canonical(ec.expected_from_hits(off, hits)), T)
    eff0 = ra.eff_lens_from_counts(counts, w["lens"])
    first = qc.run(graph, eff0, graph.uniform_start())[0]
    q, k = emu.weights(first, w["lens"], counts)
    g = _new(emu, w)(1000, 0)
    try:
        g.add_hits(off, hits)
        obs, st = g.counts(), g.stat()
        ex = g.expect(counts, T, q)
        R = emu.ratios(obs, ex)
        eff1 = g.eff_lens(counts, T, R)
    finally:
        g.close()
    eo, es = ps.classify(w, off, hits, 1000)
    ps.assert_same(obs, st, eo, es, "planted")
    assert np.array_equal(ex, ps.expect(w, counts, q)[0]) and eff1.tobytes() == ps.eff_lens(w["lens"], counts, R).tobytes()
    second = qc.run(graph, eff1, first)[0]
    err0 = float(np.abs(first - truth).sum()); err1 = float(np.abs(second - truth).sum())
    return err0, err1, {"mapped": mapped, "es": es, "fst": fst, "R": R, "graph": graph}


def test_planted_bias_is_corrected(emu, oracle_mod, lib_built, tmp_path):
    """The correction does what it is for.  Fragments are drawn from transcripts of known abundance (psb_cases.planted_transcripts:
    genes of a short and a long isoform that share a stretch, at the 3' end of the one and at the 5' end of the other, and decoys of
    their own in every length class) and each is kept with a probability that rises linearly with s / L from 0.2 to 1.0; the oracle
    maps the kept ones.  Then the steps of the CLI on the lane emulation: histogram, first estimate (quant_cases' restatement of the EM
    at the CLI's defaults), weights, observed and expected counts, ratios, effective lengths, a second estimate started from the first.
    truth_t is the number of mapped fragments that were drawn from t.  A direction, not a tolerance: sum |NumReads_t - truth_t| must
    be smaller with the correction than without, on the chosen seed.  Both sums are printed; five seeds are in DESIGN.md section 4.17."""
    err0, err1, seen = _planted(emu, tmp_path, ps.PLANTED_SEED)
    R, es = seen["R"], seen["es"]
    print("planted bias: %d fragments mapped, %d used by the sweep; R[start] over the 20 bins, mean of the classes: %s; sum |NumReads - truth| %.1f without, %.1f with the correction" % (
        int(seen["mapped"].sum()), es["used"], " ".join("%.2f" % v for v in R[0].mean(axis=0)), err0, err1))
    assert seen["mapped"].sum() > 0.95 * seen["mapped"].size and es["used"] > 3000 and seen["graph"].longest_label == 2
    early, late = R[0, :, :5].mean(), R[0, :, 10:15].mean()
    assert late > 1.5 * early                                        # the planted direction is found: starts are rarer towards the 5' end
    assert err1 < err0, (err0, err1)


def test_all_reduce_over_two_ranks(tmp_path):
    """two gloo ranks: every rank gets the sum of both ranks' counts, counts beyond 2^33 included, as uint64 in the input's shape"""
    import torch.multiprocessing as mp_
    from test_distributed_cpu import _free_port
    mp_.spawn(_all_reduce_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    exp = _rank_counts(0) + _rank_counts(1)
    assert exp.max() > 1 << 33
    for r in range(2):
        got = np.load(tmp_path / ("sum_%d.npy" % r))
        assert got.dtype == np.uint64 and got.shape == ps.SHAPE and np.array_equal(got, exp)


def _rank_counts(rank):
    c = np.random.default_rng(40 + rank).integers(0, 1 << 20, ps.SHAPE).astype(np.uint64)
    c[rank, 3 + rank, 17] = (1 << 33) + rank
    return c


def _all_reduce_worker(rank, world, port, out_dir):
    import os
    import sys
    import torch.distributed as dist
    from conftest import ROOT
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from rapmap_amd import dist as qd
    mine = _rank_counts(rank); keep = mine.copy()
    tot = qd.all_reduce_pos_counts(mine, device="cpu")
    assert np.array_equal(mine, keep)                                # the caller's array is left alone
    np.save(os.path.join(out_dir, "sum_%d.npy" % rank), tot)
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_without_a_process_group():
    from rapmap_amd import dist as qd
    c = np.arange(200, dtype=np.uint64)
    assert qd.all_reduce_pos_counts(c, device="cpu") is c


def _cli_error(extra):
    import subprocess
    import sys
    from conftest import ROOT
    return subprocess.run([sys.executable, "-m", "rapmap_amd", "quasimap", "-i", "nowhere", "-1", "a.fq", "-2", "b.fq", "-n", "--quant", "q.sf"] + extra,
                          cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_cli_rejects_pos_bias_without_fld():
    p = _cli_error(["--quantPosBias"])
    assert p.returncode == 2 and "--quantPosBias" in p.stderr and "needs --quantFLD" in p.stderr


def test_cli_rejects_pos_bias_with_gc_bias():
    p = _cli_error(["--quantFLD", "--quantPosBias", "--quantGCBias"])
    assert p.returncode == 2 and "--quantPosBias and --quantGCBias are two corrections of their own" in p.stderr


def test_cli_rejects_pos_bias_with_seq_bias():
    p = _cli_error(["--quantFLD", "--quantPosBias", "--quantSeqBias"])
    assert p.returncode == 2 and "--quantPosBias and --quantSeqBias are two corrections of their own" in p.stderr
