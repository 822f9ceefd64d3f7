"""The fragment GC bias model without a GPU: the rank structure, the observed sweep, the expected matrix and their driver
(rapmap_amd/csrc/qm_gcb.inl, qm_gcb_host.inl) under the lane emulation, and the arithmetic from the counts to effective lengths through
the built library (a pure host function).

The emulation (tests/emu/qm_emu_gcb.cpp) runs one wavefront after the other and one lane after the other, the sweep's on a tally filled
with 0xA5: it proves the LOGIC of the bodies -- the rank structure, offsets, categories, the tally, the tile table, the sliding mask
window, the reciprocal rule, the fold of a length's bins, the grid's cap -- and the driver's text, not the atomics; what contention
does to them is the GPU tests' part (test_gc_bias_gpu.py).  Every comparison is exact."""
import numpy as np
import pytest

import gcb_cases as gc
import part_cases as pc
from conftest import load_oracle
from util import pack


@pytest.fixture(scope="module")
def emu():
    import emu_gcb
    emu_gcb._lib()
    return emu_gcb


@pytest.fixture(scope="module")
def world():
    w = gc.make_world(gc.crafted_seqs())
    for a in w.values():
        a.setflags(write=False)
    # transcript starts at every kind of place within a 64-character block, a transcript across several tiles, every character class
    assert len({int(o) % 64 for o in w["off"]}) >= 12
    assert set(gc.PLAIN_LENS) | {5000} <= {int(x) for x in w["lens"]}
    assert {ord(c) for c in "ACGTacgtNn$"} <= set(w["text"].tolist())
    return w


def _new(emu, w, **caps):
    return lambda max_len, max_blocks: emu.EmuGcb(w["text"], w["off"], w["lens"], max_len, max_blocks, **caps)


def test_emulated_rank_structure(emu, world):
    g = emu.EmuGcb(world["text"], world["off"], world["lens"])
    try:
        mask, rank = g.rank_structure()
    finally:
        g.close()
    n = world["text"].size
    assert mask.size == (n + 63) // 64 + 2
    bits = np.zeros(mask.size * 64, dtype=np.uint8); bits[:n] = gc.is_gc(world["text"])
    exp_mask = np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view("<u8").ravel()
    assert np.array_equal(mask, exp_mask)
    per = bits.reshape(-1, 64).sum(axis=1)
    assert np.array_equal(rank, (np.cumsum(per) - per).astype(np.uint32)) and not mask[-2:].any()


def test_emulated_window_gc(emu, world):
    gc.check_window_gc(world, _new(emu, world))


@pytest.mark.parametrize("check", sorted(gc.EXPECT_CHECKS))
def test_emulated_expect(emu, world, check):
    gc.EXPECT_CHECKS[check](world, _new(emu, world))


@pytest.mark.parametrize("check", sorted(gc.OBS_CHECKS))
def test_emulated_observed(emu, world, check):
    gc.OBS_CHECKS[check](world, _new(emu, world))


def test_emulated_grid_cap(emu):
    L = emu._lib()
    assert L.qe_gcb_obs_grid(70001, 1) == 1 and L.qe_gcb_obs_grid(70001, 2) == 2 and L.qe_gcb_obs_grid(70001, 0) == 274 and L.qe_gcb_obs_grid(10 ** 7, 0) == 2048


@pytest.mark.parametrize("shape", sorted(pc.SHAPES))
def test_emulated_host_arrays_in_parts(emu, world, shape):
    """qm_gcb_add_hits' driver at MAX_UNITS units and MAX_ITEMS hits to a part: the same bins and counters as in one part and as the
    restatement; one fold per part"""
    off = pc.offsets_of(shape)
    hits = None
    if shape != "null":
        rng = np.random.default_rng(len(shape))
        # one record per position up to the last offset (what lies in front of offsets[0] must not be looked at), of every category a record decides
        _, hits = gc.build(world, rng.choice(np.array([gc.U, gc.U, gc.NP, gc.SS, gc.OOR, gc.OVH]), int(off[-1])), 1000, rng)
        assert hits.size == int(off[-1])
    small = _new(emu, world, max_units=pc.MAX_UNITS, max_hits=pc.MAX_ITEMS)
    whole = _new(emu, world, max_units=pc.ONE_PART, max_hits=pc.ONE_PART)
    c1, s1 = gc.fold_once(whole, off, hits)
    c, s = gc.fold_once(small, off, hits)
    eo, es = gc.classify(world, off, hits, 1000)
    gc.assert_same(c, s, eo, es, shape); gc.assert_same(c1, s1, eo, es, shape + ", one part")
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


def _index_world(idx):
    import rapmap_amd as ra
    qi = ra.QuasiIndex(idx)
    text, off = qi.arrays()
    w = {"text": text, "off": off, "lens": np.asarray(qi.txp_lens, dtype=np.int64)}
    qi.close()
    return w


def test_emulated_synth_small(emu, synth_small, oracle_mod):
    """the oracle's hits of synth_small over the index's own text: at least the fragments test_fld.py requires of the default run"""
    w = _index_world(synth_small["idx"])
    ix, orc = load_oracle(synth_small["idx"])
    q1, o1 = pack(synth_small["reads1"]); q2, o2 = pack(synth_small["reads2"])
    res = orc.map_pairs(q1, o1, q2, o2, nthreads=4)
    eo, es = gc.check_against_restatement(w, _new(emu, w), res.hit_offsets, res.hits, max_blocks=3, what="synth_small")
    assert es["units"] == 4234 and es["used"] >= 500, es
    assert np.count_nonzero(eo) >= 3
    # the expected matrix of that run's own fragment lengths
    import fld_cases as fc
    counts, _ = fc.classify(res.hit_offsets, res.hits, 1000)
    g = _new(emu, w)(1000, 0)
    try:
        H = g.expect(counts, w["lens"].size)
    finally:
        g.close()
    assert np.array_equal(H, gc.expect(w, counts))
    gc.assert_identity(w, counts, H, "synth_small")
    rs = orc.map_single(q1, o1, nthreads=4)
    eo, es = gc.check_against_restatement(w, _new(emu, w), rs.hit_offsets, rs.hits, what="single-end")
    assert es["used"] == es["same_strand"] == es["out_of_range"] == es["overhang"] == 0 and es["not_paired"] > 500 and not eo.any()


@pytest.mark.parametrize("check", sorted(gc.EFF_CHECKS))
def test_eff_lens_from_counts(lib_built, check):
    import rapmap_amd as ra
    gc.EFF_CHECKS[check](ra.gc_eff_lens_from_counts)


def test_eff_lens_agree_with_the_fragment_length_model(lib_built):
    import rapmap_amd as ra
    gc.eff_check_agrees_with_fld(ra.gc_eff_lens_from_counts, ra.eff_lens_from_counts)


def test_eff_lens_errors(lib_built):
    import rapmap_amd as ra
    c, lens, H, alpha, obs = gc.eff_inputs(5, 66)
    bad = c.copy(); bad[0] = 1
    with pytest.raises(ra.QmError, match="-1"):                      # QM_E_ARG: bin 0 is never used
        ra.gc_eff_lens_from_counts(bad, lens, H, alpha, obs)
    l0 = lens.copy(); l0[2] = 0
    with pytest.raises(ra.QmError, match="-1"):                      # QM_E_ARG: a transcript of length 0
        ra.gc_eff_lens_from_counts(c, l0, H, alpha, obs)
    with pytest.raises(ra.QmError, match="-4"):                      # QM_E_UNSUPPORTED: max_len 1024
        ra.gc_eff_lens_from_counts(np.zeros(1025, dtype=np.uint64), lens, H, alpha, obs)
    with pytest.raises(ValueError):
        ra.gc_eff_lens_from_counts(c, lens, H[:4], alpha, obs)
    eff, ex, ratio = ra.gc_eff_lens_from_counts(c, lens[:0], H[:0], alpha[:0], obs)
    assert eff.size == 0 and not ex.any() and (ratio == 1.0).all()


def test_gc_bias_file_round_trip(tmp_path):
    import rapmap_amd as ra
    rng = np.random.default_rng(3)
    obs = rng.integers(0, 1 << 40, 25).astype(np.uint64); ex = rng.random(25) * 1e7; ratio = np.clip(rng.random(25) * 3, 1e-3, 1e3); ex[4] = 0.0; ratio[4] = 1.0
    p = str(tmp_path / "q.sf.gcBias.txt")
    ra.write_gc_bias(p, obs, ex, ratio)
    lines = open(p).read().split("\n")
    assert lines[0] == "bin\tobs\texp\tratio" and len(lines) == 27 and lines[26] == "" and lines[5].startswith("4\t%d\t0\t1" % int(obs[4]))
    o, e, r = ra.read_gc_bias(p)
    assert o.dtype == np.uint64 and np.array_equal(o, obs) and e.tobytes() == ex.tobytes() and r.tobytes() == ratio.tobytes()
    open(p, "w").write("nonsense\n")
    with pytest.raises(ValueError):
        ra.read_gc_bias(p)


def test_planted_bias_is_corrected(emu, oracle_mod, lib_built, tmp_path):
    """The correction does what it is for.  Fragments are drawn from transcripts of known abundance (gcb_cases.planted_transcripts: isoform
    pairs that share half their text and differ in the GC of the rest) and each is kept with a probability that falls with its GC bin;
    the oracle maps the kept ones.  Then the steps of `quasimap --quant --quantFLD --quantGCBias`: the fragment-length histogram and
    its effective lengths, a first estimate over the class table, obs and H (the lane emulation of the sweep and of the expected
    kernel), e' through the built library, a second estimate on e' started from the first -- the EM itself is quant_cases' restatement
    at the CLI's defaults.  truth_t is the number of mapped fragments that were drawn from t: with the keep probability as the model's
    bias, P(fragment | t) = keep(bin) / sum of keep over t's windows, so the maximum-likelihood alpha_t estimates just that number, and
    a wrong effective length shows in how the shared fragments of a gene are split between its isoforms.
    A direction, not a tolerance: sum |NumReads_t - truth_t| must be smaller with the correction than without.  With the restatement
    alone (gcb_cases.classify / expect / eff_lens) the chosen seed gives 123.6 without and 65.8 with the correction, next to 61.3 with
    the planted curve itself as the ratio; four other seeds at this size: 185.5 -> 64.7, 146.2 -> 49.2, 160.3 -> 99.5, 140.9 -> 68.7."""
    import rapmap_amd as ra
    from rapmap_amd import synth
    import eqc_cases as ec
    import fld_cases as fc
    import quant_cases as qc
    names, txps, theta = gc.planted_transcripts()
    fa = str(tmp_path / "planted.fa"); synth.write_fasta(fa, names, txps)
    idx = str(tmp_path / "idx"); ra.build_index(fa, idx, threads=2)
    r1, r2, origin = gc.planted_fragments(txps, theta)
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
    assert graph.total == int(mapped.sum()) and graph.longest_label == 2
    eff0 = ra.eff_lens_from_counts(counts, w["lens"])
    first = qc.run(graph, eff0, graph.uniform_start())[0]
    g = _new(emu, w)(1000, 0)
    try:
        g.add_hits(off, hits)
        obs, st = g.counts(), g.stat()
        H = g.expect(counts, T)
    finally:
        g.close()
    eo, es = gc.classify(w, off, hits, 1000)
    gc.assert_same(obs, st, eo, es, "planted"); assert np.array_equal(H, gc.expect(w, counts))
    eff1, ex, ratio = ra.gc_eff_lens_from_counts(counts, w["lens"], H, first, obs)
    second = qc.run(graph, eff1, first)[0]
    err0 = float(np.abs(first - truth).sum()); err1 = float(np.abs(second - truth).sum())
    seen = obs > 0
    print("planted bias: %d fragments mapped, %d used by the sweep in %d bins; ratio %.3g (bin %d) .. %.3g (bin %d); sum |NumReads - truth| %.1f without, %.1f with the correction" % (
        int(mapped.sum()), es["used"], int(seen.sum()), ratio[seen][0], np.flatnonzero(seen)[0], ratio[seen][-1], np.flatnonzero(seen)[-1], err0, err1))
    assert mapped.sum() > 0.95 * mapped.size and es["used"] > 3000 and fst["used"] == es["used"] + es["overhang"]
    assert seen[6:19].all() and ratio[6:11].mean() > ratio[14:19].mean()   # the planted direction is found: GC-rich windows are under-observed
    assert err1 < err0, (err0, err1)


def test_all_reduce_over_two_ranks(tmp_path):
    """two gloo ranks: every rank gets the sum of both ranks' counts, counts beyond 2^32 included, as uint64"""
    import torch.multiprocessing as mp_
    from test_distributed_cpu import _free_port
    mp_.spawn(_all_reduce_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    exp = _rank_counts(0) + _rank_counts(1)
    assert exp.max() > 1 << 33
    for r in range(2):
        got = np.load(tmp_path / ("sum_%d.npy" % r))
        assert got.dtype == np.uint64 and got.shape == (25,) and np.array_equal(got, exp)


def _rank_counts(rank):
    c = np.random.default_rng(40 + rank).integers(0, 1 << 20, 25).astype(np.uint64)
    c[3 + rank] = (1 << 33) + rank
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
    tot = qd.all_reduce_gc_counts(mine, device="cpu")
    assert np.array_equal(mine, keep)                                # the caller's array is left alone
    np.save(os.path.join(out_dir, "sum_%d.npy" % rank), tot)
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_without_a_process_group():
    from rapmap_amd import dist as qd
    c = np.arange(25, dtype=np.uint64)
    assert qd.all_reduce_gc_counts(c, device="cpu") is c


def test_cli_rejects_gc_bias_without_fld():
    import subprocess
    import sys
    from conftest import ROOT
    p = subprocess.run([sys.executable, "-m", "rapmap_amd", "quasimap", "-i", "nowhere", "-1", "a.fq", "-2", "b.fq", "-n", "--quant", "q.sf", "--quantGCBias"],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 2 and "--quantGCBias" in p.stderr and "needs --quantFLD" in p.stderr
