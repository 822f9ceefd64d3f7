"""The fragment-length distribution without a GPU: the sweep and its driver (rapmap_amd/csrc/qm_fld.inl, qm_fld_host.inl) under the lane
emulation, the arithmetic from histogram to effective lengths through the built library (a pure host function), the file format, the
all-reduce, the CLI's checks.

The emulation (tests/emu/qm_emu_fld.cpp) runs one wavefront after the other and one lane after the other, each on a slab filled with
0xA5: it proves the LOGIC of the sweep -- offsets, categories, the slab, the flush, the grid's cap -- and the driver's text (folds,
add_counts, clear, the parts of host arrays), not the atomics; what contention
does to them is the GPU tests' part (test_fld_gpu.py).  Every comparison is exact."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import fld_cases as fc
import part_cases as pc
from conftest import ROOT, load_oracle
from util import pack


@pytest.fixture(scope="module")
def emu():
    import emu_fld
    emu_fld._lib()
    return emu_fld


@pytest.mark.parametrize("check", sorted(fc.CHECKS))
def test_emulated_crafted(emu, check):
    fc.CHECKS[check](emu.EmuFld)


def test_emulated_grid_cap(emu):
    L = emu._lib()
    assert L.qe_fld_grid(70001, 1) == 1 and L.qe_fld_grid(70001, 2) == 2 and L.qe_fld_grid(70001, 0) == 274 and L.qe_fld_grid(10 ** 7, 0) == 2048
    assert L.qe_fld_grid(1, 0) == 1 and L.qe_fld_grid(257, 0) == 2


def _part_hits(off, rng):
    """records for offsets that may start above 0 (what lies in front is random and must not be looked at); every third: not paired"""
    off_, h = fc.build(np.full(int(off[-1]), fc.U), 1000, rng)
    h["mate_status"][::3] = 1
    return h


@pytest.mark.parametrize("shape", sorted(pc.SHAPES))
def test_emulated_host_arrays_in_parts(emu, shape):
    """qm_fld_add_hits' driver at MAX_UNITS units and MAX_ITEMS hits to a part: the same bins and counters as in one part and as the
    restatement; one fold per part"""
    off = pc.offsets_of(shape)
    hits = None if shape == "null" else _part_hits(off, np.random.default_rng(len(shape)))
    small = lambda max_len, max_blocks: emu.EmuFld(max_len, max_blocks, pc.MAX_UNITS, pc.MAX_ITEMS)
    whole = lambda max_len, max_blocks: emu.EmuFld(max_len, max_blocks, pc.ONE_PART, pc.ONE_PART)
    c1, s1 = fc.fold_once(whole, off, hits)
    c, s = fc.fold_once(small, off, hits)
    ec, es = fc.classify(off, hits, 1000)
    fc.assert_same(c, s, ec, es, shape); fc.assert_same(c1, s1, ec, es, shape + ", one part")
    assert s["folds"] == len(pc.parts(off)) and s1["folds"] == min(len(off) - 1, 1)
    assert s["last_fold_us"] == 0


def test_emulated_decreasing_offsets_leave_the_object_alone(emu):
    off, h = fc.random_batch(300, 1000, seed=3)
    f = emu.EmuFld(1000, 0, pc.MAX_UNITS, pc.MAX_ITEMS)
    try:
        f.add_hits(off, h)
        before = (f.counts(), f.stat())
        with pytest.raises(emu.ArgError):
            f.add_hits(pc.decreasing(), h)
        assert np.array_equal(f.counts(), before[0]) and f.stat() == before[1]
    finally:
        f.close()


SMALL_VARIANTS = {"default": {}, "fuzzy": {"fuzzy": 1}, "no_dovetail": {"noDovetail": 1}, "sel_aln": {"selAln": 1}}


@pytest.mark.parametrize("variant", sorted(SMALL_VARIANTS))
def test_emulated_synth_small(emu, synth_small, oracle_mod, variant):
    ix, orc = load_oracle(synth_small["idx"])
    q1, o1 = pack(synth_small["reads1"]); q2, o2 = pack(synth_small["reads2"])
    res = orc.map_pairs(q1, o1, q2, o2, opts=oracle_mod.default_opts(**SMALL_VARIANTS[variant]), nthreads=4)
    ec, es = fc.check_against_restatement(emu.EmuFld, res.hit_offsets, res.hits, max_blocks=3, what="synth_small, " + variant)
    assert es["units"] == 4234
    if variant == "default":
        assert es["used"] >= 500, es                                 # (about 950 uniquely and properly paired units: no empty histogram)


def test_emulated_sample_data(emu, sample_data, oracle_mod):
    ix, orc = load_oracle(sample_data["idx"])
    q1, o1 = pack(sample_data["reads1"]); q2, o2 = pack(sample_data["reads2"])
    res = orc.map_pairs(q1, o1, q2, o2, nthreads=4)
    ec, es = fc.check_against_restatement(emu.EmuFld, res.hit_offsets, res.hits, what="sample_data")
    assert es["used"] >= 5000, es                                    # (about 6 900)


def test_emulated_single_end(emu, synth_small, oracle_mod):
    """a single-end batch is valid: every mapped unit is not_paired"""
    ix, orc = load_oracle(synth_small["idx"])
    q1, o1 = pack(synth_small["reads1"])
    res = orc.map_single(q1, o1, nthreads=4)
    ec, es = fc.check_against_restatement(emu.EmuFld, res.hit_offsets, res.hits, what="single-end")
    assert es["used"] == es["same_strand"] == es["out_of_range"] == 0 and es["not_paired"] > 500 and not ec.any()


@pytest.mark.parametrize("check", sorted(fc.EFF_CHECKS))
def test_eff_lens_from_counts(lib_built, check):
    import rapmap_amd as ra
    fc.EFF_CHECKS[check](ra.eff_lens_from_counts, ra.QmError)


def test_mean_and_file_round_trip(tmp_path):
    import rapmap_amd as ra
    rng = np.random.default_rng(3)
    c = np.zeros(1001, dtype=np.uint64); c[150:600] = rng.integers(0, 1 << 30, 450).astype(np.uint64); c[1000] = 1
    used = int(c.sum())
    p = str(tmp_path / "q.sf.flenDist.txt")
    ra.write_flen_dist(p, c)
    text = open(p).read()
    assert text.endswith("\n") and text.count("\n") == 1 and text.count("\t") == 1000
    back = ra.read_flen_dist(p)
    assert back.dtype == np.float64 and back.size == 1001 and back[0] == 0
    assert [float(w) for w in text.split()] == [int(x) / used for x in c]          # %.17g gives every double back
    assert np.array_equal(np.rint(back * used).astype(np.uint64), c)
    assert ra.frag_len_mean(c) == sum(l * int(c[l]) for l in range(1001)) / used
    empty = np.zeros(3, dtype=np.uint64)
    ra.write_flen_dist(p, empty)
    assert open(p).read() == "0\t0\t0\n" and not ra.read_flen_dist(p).any()
    assert np.isnan(ra.frag_len_mean(empty))


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _reduce_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from rapmap_amd import dist as qd
    c = np.arange(1001, dtype=np.uint64) * np.uint64(rank + 1); c[0] = 0; c[7] = (1 << 40) + rank
    tot = qd.all_reduce_frag_len_counts(c, device="cpu")
    np.save(os.path.join(out_dir, "fld_%d.npy" % rank), tot)
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_two_ranks(tmp_path):
    import torch.multiprocessing as mp_
    mp_.spawn(_reduce_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    exp = np.arange(1001, dtype=np.uint64) * np.uint64(3); exp[0] = 0; exp[7] = (1 << 41) + 1
    for r in range(2):
        got = np.load(tmp_path / ("fld_%d.npy" % r))
        assert got.dtype == np.uint64 and np.array_equal(got, exp)


def test_all_reduce_without_a_process_group():
    from rapmap_amd import dist as qd
    c = np.arange(1001, dtype=np.uint64)
    assert qd.all_reduce_frag_len_counts(c, device="cpu") is c


@pytest.mark.parametrize("extra,reads,why", [([], "paired", "needs --quant"), (["--quant", "q.sf", "--quantFragLenMean", "200"], "paired", "not together with"),
                                             (["--quant", "q.sf"], "single", "needs paired-end reads")])
def test_cli_rejects_quant_fld(extra, reads, why):
    r = ["-1", "a.fq", "-2", "b.fq"] if reads == "paired" else ["-r", "a.fq"]
    p = subprocess.run([sys.executable, "-m", "rapmap_amd", "quasimap", "-i", "nowhere", "--quantFLD", "-n"] + r + extra,
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 2 and "--quantFLD" in p.stderr and why in p.stderr
