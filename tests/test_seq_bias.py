"""The sequence-specific bias model without a GPU: the contexts, the observed sweep, the expected counts, the effective lengths and
their driver (rapmap_amd/csrc/qm_sqb.inl, qm_sqb_host.inl) under the lane emulation, and the two pure host functions (weights, ratios)
through the built library and through the emulation's build of the same text.

The emulation (tests/emu/qm_emu_sqb.cpp) runs one wavefront after the other and one lane after the other, every slab filled with
0xA5: it proves the LOGIC of the bodies -- contexts, categories, the tally, the tile table, the ballots of the expected kernel, the
ring of the effective-length kernel as it slides and wraps, the order of every float sum, the grid's cap -- and the driver's text,
not the atomics; what contention does to them is the GPU tests' part (test_seq_bias_gpu.py).  Every comparison is exact."""
import numpy as np
import pytest

import gcb_cases as gc
import part_cases as pc
import sqb_cases as sq
from conftest import load_oracle
from util import pack


@pytest.fixture(scope="module")
def emu():
    import emu_sqb
    emu_sqb._lib()
    return emu_sqb


@pytest.fixture(scope="module")
def world():
    w = gc.make_world(sq.crafted_seqs())
    for a in w.values():
        a.setflags(write=False)
    assert set(sq.LENS) <= {int(x) for x in w["lens"]} and {ord(c) for c in "ACGTacgtNn$"} <= set(w["text"].tolist())
    return w


def _new(emu, w, **caps):
    return lambda max_len, max_blocks: emu.EmuSqb(w["text"], w["off"], w["lens"], max_len, max_blocks, **caps)


def test_emulated_contexts(emu, world):
    sq.check_contexts(world, _new(emu, world))
    # by hand, on ACGTACGTAC: the 5' context of start 3 is characters 0 .. 8, ACGTACGTA; the 3' context of last position 5 is
    # characters 8 .. 0 complemented, TACGTACGT
    w = gc.make_world([b"ACGTACGTAC", b"acgtacgtac", b"ACGTNCGTAC"])
    g = _new(emu, w)(1000, 0)
    try:
        got = g.context([0, 1, 2, 0, 0, 0], [3, 3, 3, 5, 6, 7], [0, 0, 0, 1, 1, 1])
    finally:
        g.close()
    five = [0, 1, 6, 27, 44, 49, 6, 27, 44]                          # A, AC, ACG, CGT, GTA, TAC, ACG, CGT, GTA
    three = [3, 12, 49, 6, 27, 44, 49, 6, 27]                        # T, TA, TAC, ACG, CGT, GTA, TAC, ACG, CGT
    assert got[0].tolist() == five and got[1].tolist() == five and (got[2] == -1).all()
    assert got[3].tolist() == three and (got[4] >= 0).all() and (got[5] == -1).all()


@pytest.mark.parametrize("check", sorted(sq.OBS_CHECKS))
def test_emulated_observed(emu, world, check):
    sq.OBS_CHECKS[check](world, _new(emu, world))


def test_emulated_ambiguous_units(emu, world):
    """a fragment whose context holds N or n is `ambiguous`, not used, and one that hangs over is `overhang` first"""
    lens = [int(x) for x in world["lens"]]
    t = len(lens) - 1                                                # ACGTACGTA N ACGTACGTA
    assert lens[t] == 19
    rows = [(sq._one(t, 3, 3, 3), "used"),                           # both contexts are characters 0 .. 8
            (sq._one(t, 4, 4, 3), "ambiguous"), (sq._one(t, 12, 12, 3), "ambiguous"),   # characters 1 .. 9, 9 .. 17
            (sq._one(t, 2, 2, 9), "overhang"), (sq._one(t, 13, 13, 4), "overhang")]     # the N lies in the 3' context, but s = 2; i = 16 = L - 3
    h = np.concatenate([r[0] for r in rows]); off = np.arange(len(rows) + 1, dtype=np.int64)
    for rec, cat in rows:
        assert sq.classify(world, [0, 1], rec, 1000)[1][cat] == 1, cat
    eo, es = sq.check_against_restatement(world, _new(emu, world), off, h, what="N in a context")
    assert es["ambiguous"] == 2 and es["used"] == 1 and es["overhang"] == 2


def test_emulated_grid_cap(emu):
    L = emu._lib()
    assert L.qe_sqb_obs_grid(70001, 1) == 1 and L.qe_sqb_obs_grid(70001, 2) == 2 and L.qe_sqb_obs_grid(70001, 0) == 274 and L.qe_sqb_obs_grid(10 ** 7, 0) == 2048
    assert L.qe_sqb_tile_grid(10 ** 7, 0) == 1024 and L.qe_sqb_tile_grid(5, 0) == 2 and L.qe_sqb_tile_grid(5, 1) == 1


@pytest.mark.parametrize("shape", sorted(pc.SHAPES))
def test_emulated_host_arrays_in_parts(emu, world, shape):
    """qm_sqb_add_hits' driver at MAX_UNITS units and MAX_ITEMS hits to a part: the same counts and counters as in one part and as the
    restatement; one fold per part"""
    off = pc.offsets_of(shape)
    hits = None
    if shape != "null":
        rng = np.random.default_rng(len(shape))
        _, hits = gc.build(world, rng.choice(np.array([gc.U, gc.U, gc.NP, gc.SS, gc.OOR, gc.OVH]), int(off[-1])), 1000, rng)
        assert hits.size == int(off[-1])
    small = _new(emu, world, max_units=pc.MAX_UNITS, max_hits=pc.MAX_ITEMS)
    whole = _new(emu, world, max_units=pc.ONE_PART, max_hits=pc.ONE_PART)
    c1, s1 = sq.fold_once(whole, off, hits)
    c, s = sq.fold_once(small, off, hits)
    eo, es = sq.classify(world, off, hits, 1000)
    sq.assert_same(c, s, eo, es, shape); sq.assert_same(c1, s1, eo, es, shape + ", one part")
    assert s["folds"] == len(pc.parts(off)) and s1["folds"] == min(len(off) - 1, 1)


def test_emulated_decreasing_offsets_leave_the_object_alone(emu, world):
    off, h = sq.random_batch(world, 300, 1000, seed=3)
    f = _new(emu, world, max_units=pc.MAX_UNITS, max_hits=pc.MAX_ITEMS)(1000, 0)
    try:
        f.add_hits(off, h)
        before = (f.counts(), f.stat())
        with pytest.raises(emu.ArgError):
            f.add_hits(pc.decreasing(), h)
        assert np.array_equal(f.counts(), before[0]) and f.stat() == before[1]
    finally:
        f.close()


@pytest.mark.parametrize("check", sorted(sq.EXPECT_CHECKS))
def test_emulated_expect(emu, world, check):
    sq.EXPECT_CHECKS[check](world, _new(emu, world))


@pytest.mark.parametrize("check", sorted(sq.EFF_CHECKS))
def test_emulated_eff_lens(emu, world, lib_built, check):
    if check == "ratio_one":
        import rapmap_amd as ra
        sq.check_eff_ratio_one(world, _new(emu, world), ra.eff_lens_from_counts)
    else:
        sq.EFF_CHECKS[check](world, _new(emu, world))


def test_weights(emu, lib_built):
    import rapmap_amd as ra
    sq.check_weights(ra.seq_bias_weights)
    sq.check_weights(emu.weights)


def test_weights_errors(lib_built):
    import rapmap_amd as ra
    alpha, lens, c = sq.weight_inputs(5, 76)
    bad = c.copy(); bad[0] = 1
    with pytest.raises(ra.QmError, match="-1"):                      # QM_E_ARG: bin 0 is never used
        ra.seq_bias_weights(alpha, lens, bad)
    l0 = lens.copy(); l0[2] = 0
    with pytest.raises(ra.QmError, match="-1"):                      # QM_E_ARG: a transcript of length 0
        ra.seq_bias_weights(alpha, l0, c)
    with pytest.raises(ra.QmError, match="-4"):                      # QM_E_UNSUPPORTED: max_len 1024
        ra.seq_bias_weights(alpha, lens, np.zeros(1025, dtype=np.uint64))
    a = alpha.copy(); a[1] = np.inf
    with pytest.raises(ra.QmError, match="-1"):                      # QM_E_ARG: not finite
        ra.seq_bias_weights(a, lens, c)
    with pytest.raises(ValueError):
        ra.seq_bias_weights(alpha[:4], lens, c)
    q, k = ra.seq_bias_weights(alpha[:0], lens[:0], c)
    assert q.size == 0 and k == 0


def test_ratios(emu, lib_built):
    import rapmap_amd as ra
    sq.check_ratios(ra.seq_bias_ratios)
    sq.check_ratios(emu.ratios)
    with pytest.raises(ValueError):
        ra.seq_bias_ratios(np.zeros(25, dtype=np.uint64), np.zeros(1152, dtype=np.uint64))


def test_seq_bias_file_round_trip(tmp_path):
    import rapmap_amd as ra
    rng = np.random.default_rng(3)
    obs = rng.integers(0, 1 << 40, sq.SHAPE).astype(np.uint64); ex = rng.integers(0, 1 << 62, sq.SHAPE).astype(np.uint64); ex[1, 8, 63] = 2 ** 64 - 1
    ratio = np.exp2(rng.uniform(-2, 2, sq.SHAPE)); ratio[0, 0, 4:] = 1.0
    p = str(tmp_path / "q.sf.seqBias.txt")
    ra.write_seq_bias(p, obs, ex, ratio)
    lines = open(p).read().split("\n")
    assert lines[0] == "end\tposition\tword\tobs\texp\tratio" and len(lines) == 1154 and lines[1153] == "" and lines[6].startswith("0\t0\t5\t%d\t%d\t1" % (int(obs[0, 0, 5]), int(ex[0, 0, 5])))
    assert lines[1152].startswith("1\t8\t63\t")
    o, e, r = ra.read_seq_bias(p)
    assert o.dtype == np.uint64 and np.array_equal(o, obs) and e.dtype == np.uint64 and np.array_equal(e, ex) and r.tobytes() == ratio.tobytes()
    open(p, "w").write("nonsense\n")
    with pytest.raises(ValueError):
        ra.read_seq_bias(p)


def _index_world(idx):
    import rapmap_amd as ra
    qi = ra.QuasiIndex(idx)
    text, off = qi.arrays()
    w = {"text": text, "off": off, "lens": np.asarray(qi.txp_lens, dtype=np.int64)}
    qi.close()
    return w


def test_emulated_synth_small(emu, synth_small, oracle_mod):
    """the oracle's hits of synth_small over the index's own text; then that run's own histogram and weights through the expected counts,
    the ratios and the effective lengths"""
    import fld_cases as fc
    w = _index_world(synth_small["idx"])
    ix, orc = load_oracle(synth_small["idx"])
    q1, o1 = pack(synth_small["reads1"]); q2, o2 = pack(synth_small["reads2"])
    res = orc.map_pairs(q1, o1, q2, o2, nthreads=4)
    eo, es = sq.check_against_restatement(w, _new(emu, w), res.hit_offsets, res.hits, max_blocks=3, what="synth_small")
    assert es["units"] == 4234 and es["used"] >= 500, es
    counts, _ = fc.classify(res.hit_offsets, res.hits, 1000)
    T = w["lens"].size
    alpha = np.random.default_rng(5).random(T) * 50
    q, k = emu.weights(alpha, w["lens"], counts)
    assert np.array_equal(q, sq.weights(alpha, w["lens"], counts)[0]) and sq.weight_bound(q, w["lens"], counts) < 2 ** 63
    g = _new(emu, w)(1000, 0)
    try:
        ex = g.expect(counts, T, q)
        exp, totals = sq.expect(w, counts, q)
        assert np.array_equal(ex, exp)
        sq.assert_nine_sums(ex, totals, "synth_small")
        R = emu.ratios(eo, ex)
        assert R.tobytes() == sq.ratios(eo, ex).tobytes() and (R != 1.0).any()
        e = g.eff_lens(counts, T, R)
        assert e.tobytes() == sq.eff_lens(w, counts, R).tobytes()
    finally:
        g.close()
    rs = orc.map_single(q1, o1, nthreads=4)
    eo, es = sq.check_against_restatement(w, _new(emu, w), rs.hit_offsets, rs.hits, what="single-end")
    assert es["used"] == es["same_strand"] == es["out_of_range"] == es["overhang"] == es["ambiguous"] == 0 and es["not_paired"] > 500 and not eo.any()


def _planted(emu, tmp_path, seed):
    """the steps of `quasimap --quant --quantFLD --quantSeqBias` on fragments with a planted bias -> (err0, err1, what was seen)"""
    import rapmap_amd as ra
    from rapmap_amd import synth
    import eqc_cases as ec
    import fld_cases as fc
    import quant_cases as qc
    names, txps, theta = sq.planted_transcripts(seed)
    fa = str(tmp_path / ("planted%d.fa" % seed)); synth.write_fasta(fa, names, txps)
    idx = str(tmp_path / ("idx%d" % seed)); ra.build_index(fa, idx, threads=2)
    r1, r2, origin = sq.planted_fragments(txps, theta, seed=seed + 1)
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
    eo, es = sq.classify(w, off, hits, 1000)
    sq.assert_same(obs, st, eo, es, "planted")
    assert np.array_equal(ex, sq.expect(w, counts, q)[0]) and eff1.tobytes() == sq.eff_lens(w, counts, R).tobytes()
    second = qc.run(graph, eff1, first)[0]
    err0 = float(np.abs(first - truth).sum()); err1 = float(np.abs(second - truth).sum())
    return err0, err1, {"mapped": mapped, "es": es, "fst": fst, "R": R, "graph": graph}


def test_planted_bias_is_corrected(emu, oracle_mod, lib_built, tmp_path):
    """The correction does what it is for.  Fragments are drawn from transcripts of known abundance (sqb_cases.planted_transcripts:
    isoform pairs that share part of their text and differ in how often the favoured start, a G, occurs in the rest) and each is kept
    with a probability that depends on its 5' context: 1 when it begins with G, a quarter otherwise; the oracle maps the kept ones.
    Then the steps of the CLI on the lane emulation: histogram, first estimate (quant_cases' restatement of the EM at the CLI's
    defaults), weights, observed and expected counts, ratios, effective lengths, a second estimate started from the first.
    truth_t is the number of mapped fragments that were drawn from t.  A direction, not a tolerance: sum |NumReads_t - truth_t| must
    be smaller with the correction than without, on the chosen seed.  Both sums are printed; five seeds are in DESIGN.md section 4.16."""
    err0, err1, seen = _planted(emu, tmp_path, sq.PLANTED_SEED)
    R, es = seen["R"], seen["es"]
    print("planted bias: %d fragments mapped, %d used by the sweep; R[5'][j = 3] for A C G T after any two characters: %s; sum |NumReads - truth| %.1f without, %.1f with the correction" % (
        int(seen["mapped"].sum()), es["used"], " ".join("%.3g" % R[0, 3].reshape(16, 4)[:, c].mean() for c in range(4)), err0, err1))
    assert seen["mapped"].sum() > 0.95 * seen["mapped"].size and es["used"] > 3000 and seen["graph"].longest_label == 2
    by_char = R[0, 3].reshape(16, 4).mean(axis=0)                    # j = 3 is the fragment's first character
    assert by_char[2] > 1.5 * max(by_char[0], by_char[1], by_char[3])   # the planted direction is found
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
        assert got.dtype == np.uint64 and got.shape == sq.SHAPE and np.array_equal(got, exp)


def _rank_counts(rank):
    c = np.random.default_rng(40 + rank).integers(0, 1 << 20, sq.SHAPE).astype(np.uint64)
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
    tot = qd.all_reduce_seq_counts(mine, device="cpu")
    assert np.array_equal(mine, keep)                                # the caller's array is left alone
    np.save(os.path.join(out_dir, "sum_%d.npy" % rank), tot)
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_without_a_process_group():
    from rapmap_amd import dist as qd
    c = np.arange(1152, dtype=np.uint64)
    assert qd.all_reduce_seq_counts(c, device="cpu") is c


def _cli_error(extra):
    import subprocess
    import sys
    from conftest import ROOT
    return subprocess.run([sys.executable, "-m", "rapmap_amd", "quasimap", "-i", "nowhere", "-1", "a.fq", "-2", "b.fq", "-n", "--quant", "q.sf"] + extra,
                          cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_cli_rejects_seq_bias_without_fld():
    p = _cli_error(["--quantSeqBias"])
    assert p.returncode == 2 and "--quantSeqBias" in p.stderr and "needs --quantFLD" in p.stderr


def test_cli_rejects_seq_bias_with_gc_bias():
    p = _cli_error(["--quantFLD", "--quantSeqBias", "--quantGCBias"])
    assert p.returncode == 2 and "--quantSeqBias" in p.stderr and "--quantGCBias" in p.stderr
