"""The library type without a GPU: the sweep and its driver (rapmap_amd/csrc/qm_lib.inl, qm_lib_host.inl) under the lane emulation, the
pure host functions (type masks, inference) through the built library, the JSON file, the all-reduce, the CLI's checks.

The emulation (tests/emu/qm_emu_lib.cpp) runs one wavefront after the other and one lane after the other, on scratch filled with 0xA5:
it proves the LOGIC of the sweep -- codes, ballots, the scan's use, the compaction, the unit offsets, the grid's cap -- and the driver's
text, not the atomics; what contention does to them is the GPU tests' part (test_lib_format_gpu.py).  Every comparison is exact."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import lib_cases as lc
import part_cases as pc
from conftest import ROOT, load_oracle
from util import pack


@pytest.fixture(scope="module")
def emu():
    import emu_lib
    emu_lib._lib()
    return emu_lib


@pytest.mark.parametrize("check", sorted(lc.CHECKS))
def test_emulated_crafted(emu, check):
    lc.CHECKS[check](emu.EmuLib)


def test_emulated_grid_cap(emu):
    L = emu._lib()
    assert L.qe_lib_grid(70001, 1) == 1 and L.qe_lib_grid(70001, 2) == 2 and L.qe_lib_grid(70001, 0) == 274 and L.qe_lib_grid(10 ** 7, 0) == 2048
    assert L.qe_lib_grid(0, 0) == 1 and L.qe_lib_grid(1, 0) == 1 and L.qe_lib_grid(257, 0) == 2


@pytest.mark.parametrize("shape", sorted(pc.SHAPES))
def test_emulated_host_arrays_in_parts(emu, shape):
    """qm_lib_add_hits' and qm_lib_compact_hits' driver at MAX_UNITS units and MAX_ITEMS hits to a part: the same tallies as in one
    part and as the restatement, the parts' filtered lists joined into the restatement's; one sweep per part"""
    off = pc.offsets_of(shape)
    rng = np.random.default_rng(len(shape))
    hits = None if shape == "null" else lc.records(lc.random_codes(int(off[-1]), rng, every_wave=False), rng)
    small = lambda t, mb: emu.EmuLib(t, mb, pc.MAX_UNITS, pc.MAX_ITEMS)
    whole = lambda t, mb: emu.EmuLib(t, mb, pc.ONE_PART, pc.ONE_PART)
    for t in ("ISF", "IU", "A"):
        ew, eo, et = lc.check_against_restatement(small, off, hits, t, what=shape)
        lc.check_against_restatement(whole, off, hits, t, what=shape + ", one part")
        a = small(t, 0); b = small(t, 0); w = whole(t, 0)
        a.add_hits(off, hits); no, tids = b.compact_hits(off, hits); no1, tids1 = w.compact_hits(off, hits)
        assert a.stat()["sweeps"] == b.stat()["sweeps"] == len(pc.parts(off)) and w.stat()["sweeps"] == min(len(off) - 1, 1)
        assert np.array_equal(no, no1) and np.array_equal(tids, tids1) and np.array_equal(a.counts(), w.counts()) and np.array_equal(b.counts(), w.counts())
        assert no[0] == 0 and len(no) == len(off) and int(no[-1]) == tids.size == int(ew[lc.W_KEPT_HITS])


def test_emulated_decreasing_offsets_leave_the_object_alone(emu):
    off, h = lc.random_batch(300, seed=3)
    for compact in (False, True):
        f = emu.EmuLib("ISF", 0, pc.MAX_UNITS, pc.MAX_ITEMS)
        f.add_hits(off, h)
        before = (f.counts(), f.stat())
        with pytest.raises(emu.ArgError):
            (f.compact_hits if compact else f.add_hits)(pc.decreasing(), h)
        assert np.array_equal(f.counts(), before[0]) and f.stat() == before[1]


def test_emulated_bad_mask(emu):
    for m in (0, 0x1000, 0xffff):
        with pytest.raises(emu.ArgError):
            emu.EmuLib(m)


@pytest.mark.parametrize("lib_type", sorted(lc.TYPES) + [1 << lc.LR])
def test_emulated_eqc_add_lib(emu, lib_type):
    """qm_eqc_add_lib's fold: under the all-codes mask the table of the plain fold, under every other mask the dictionary of the
    filtered lists; the tallies are the sweep's"""
    import emu_eqc
    for name, off, h in lc.eqc_batches():
        ew, eo, et = lc.tally(off, h, lib_type)
        table, ctr = emu.eqc_add_lib(off, h, lib_type, max_blocks=3)
        lc.assert_same(ctr, ew, lib_type, name)
        if lc.mask_of(lib_type) == lc.ALL_CODES:
            plain = emu_eqc.run(off, h["tid"])[:3]
            for x, y in zip(table, plain):
                assert x.tobytes() == y.tobytes(), name
            assert lc.table_classes(*table) == lc.filtered_classes(off, h["tid"])
        else:
            assert lc.table_classes(*table) == lc.filtered_classes(eo, et), name
            assert sum(lc.table_classes(*table).values()) == int(ew[lc.W_KEPT])


SMALL_VARIANTS = {"default": {}, "fuzzy": {"fuzzy": 1}, "no_dovetail": {"noDovetail": 1}, "sel_aln": {"selAln": 1}}


@pytest.fixture(scope="module")
def small_pairs(synth_small):
    q1, o1 = pack(synth_small["reads1"]); q2, o2 = pack(synth_small["reads2"])
    return q1, o1, q2, o2


@pytest.mark.parametrize("variant", sorted(SMALL_VARIANTS))
def test_emulated_synth_small(emu, synth_small, small_pairs, oracle_mod, variant):
    ix, orc = load_oracle(synth_small["idx"])
    res = orc.map_pairs(*small_pairs, opts=oracle_mod.default_opts(**SMALL_VARIANTS[variant]), nthreads=4)
    for t in ("ISF", "ISR", "IU", "A"):
        ew, eo, et = lc.check_against_restatement(emu.EmuLib, res.hit_offsets, res.hits, t, max_blocks=3, what="synth_small, " + variant)
        assert int(ew[lc.W_UNITS]) == 4234
        if variant == "default" and t in ("ISF", "ISR"):
            assert int(ew[lc.W_KEPT]) >= 1500 and int(ew[lc.W_DROPPED]) >= 1500, ew.tolist()
    if variant == "default":
        assert lc.infer(ew) == "IU"


def test_emulated_sample_data(emu, sample_data, oracle_mod):
    ix, orc = load_oracle(sample_data["idx"])
    q1, o1 = pack(sample_data["reads1"]); q2, o2 = pack(sample_data["reads2"])
    res = orc.map_pairs(q1, o1, q2, o2, nthreads=4)
    for t in ("ISF", "ISR"):
        ew, _, _ = lc.check_against_restatement(emu.EmuLib, res.hit_offsets, res.hits, t, what="sample_data")
        assert int(ew[lc.W_KEPT]) >= 4000 and int(ew[lc.W_DROPPED]) >= 4000, ew.tolist()
    assert lc.infer(ew) == "IU"


def test_emulated_single_end(emu, synth_small, small_pairs, oracle_mod):
    """a single-end call is tallied in codes 10 and 11 only, and U keeps all of it"""
    ix, orc = load_oracle(synth_small["idx"])
    res = orc.map_single(small_pairs[0], small_pairs[1], nthreads=4)
    ew, eo, et = lc.check_against_restatement(emu.EmuLib, res.hit_offsets, res.hits, "U", what="single-end")
    assert int(ew[:10].sum()) == 0 and int(ew[lc.SF]) > 500 and int(ew[lc.SR]) > 500 and int(ew[lc.W_OTHER]) == 0
    assert int(ew[lc.W_KEPT_HITS]) == int(ew[lc.W_HITS]) == len(res.hits) and int(ew[lc.W_DROPPED]) == 0 and np.array_equal(eo, res.hit_offsets)
    ew, _, _ = lc.check_against_restatement(emu.EmuLib, res.hit_offsets, res.hits, "IU", what="single-end")
    assert int(ew[lc.W_KEPT]) == 0 and int(ew[lc.W_DROPPED]) > 500


# ---- the pure host functions, through the built library

def test_type_masks(lib_built):
    import rapmap_amd as ra
    assert set(ra.LIB_TYPES) == set(lc.TYPES) and ra.LIB_CODES == lc.CODES
    for t in ra.LIB_TYPES:
        assert ra.lib_type_mask(t) == lc.mask_of(t), t
    assert ra.lib_type_mask("A") == ra.LIB_ALL_CODES == 0xfff
    for bad in ("", "isf", "IS", "ISFX", "AU", " A", "UU"):
        with pytest.raises(ra.QmError, match="-1"):                  # QM_E_ARG
            ra.lib_type_mask(bad)


def test_infer(lib_built):
    import rapmap_amd as ra
    lc.check_infer(ra.infer_lib_type)


def test_infer_bound(lib_built):
    """counts below 2^59 are taken, one at 2^59 is QM_E_UNSUPPORTED, whichever single-hit word holds it"""
    import rapmap_amd as ra
    for w in range(12, 24):
        c = np.zeros(32, dtype=np.uint64); c[w] = 2 ** 59
        with pytest.raises(ra.QmError, match="-4"):
            ra.infer_lib_type(c)
        c[w] = 2 ** 59 - 1
        assert ra.infer_lib_type(c) == lc.infer(c)
    c = np.zeros(32, dtype=np.uint64); c[:12] = 2 ** 62; c[24:31] = 2 ** 62   # only words 12 .. 23 are looked at
    assert ra.infer_lib_type(c) == ""
    with pytest.raises(ValueError):
        ra.infer_lib_type(np.zeros(31, dtype=np.uint64))


def test_json_round_trip(lib_built, tmp_path):
    import json
    import rapmap_amd as ra
    off, h = lc.random_batch(4097, seed=51)
    for t in ("ISF", "A"):
        w, _, _ = lc.tally(off, h, t)
        p = str(tmp_path / ("q.sf.%s.lib_format_counts.json" % t))
        ra.write_lib_format_counts(p, w, t)
        back, d = ra.read_lib_format_counts(p)
        assert np.array_equal(back, w) and d == json.load(open(p))
        assert d["inferred_format"] == lc.infer(w) and d["expected_format"] == (t if t != "A" else lc.infer(w))
        assert d["compatible_fragment_ratio"] == int(w[26]) / (int(w[26]) + int(w[27]))
        assert list(d["hits_by_code"]) == list(lc.CODES) and d["kept_units"] == int(w[26]) and d["other_hits"] == int(w[30])
    ra.write_lib_format_counts(p, np.zeros(32, dtype=np.uint64), "A")
    assert ra.read_lib_format_counts(p)[1]["compatible_fragment_ratio"] == 0.0 and ra.read_lib_format_counts(p)[1]["expected_format"] == ""


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _reduce_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from rapmap_amd import dist as qd
    c = np.arange(32, dtype=np.uint64) * np.uint64(rank + 1); c[31] = 0; c[7] = (1 << 40) + rank
    tot = qd.all_reduce_lib_counts(c, device="cpu")
    np.save(os.path.join(out_dir, "lib_%d.npy" % rank), tot)
    dist.barrier()
    dist.destroy_process_group()


def test_all_reduce_two_ranks(tmp_path):
    import torch.multiprocessing as mp_
    mp_.spawn(_reduce_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    exp = np.arange(32, dtype=np.uint64) * np.uint64(3); exp[31] = 0; exp[7] = (1 << 41) + 1
    for r in range(2):
        got = np.load(tmp_path / ("lib_%d.npy" % r))
        assert got.dtype == np.uint64 and np.array_equal(got, exp)


def test_all_reduce_without_a_process_group():
    from rapmap_amd import dist as qd
    c = np.arange(32, dtype=np.uint64)
    assert qd.all_reduce_lib_counts(c, device="cpu") is c


@pytest.mark.parametrize("lib_type,reads,why", [("ISF", "single", "needs paired-end reads"), ("IU", "single", "needs paired-end reads"),
                                                ("MSR", "single", "needs paired-end reads"), ("U", "paired", "not with paired-end reads"),
                                                ("SF", "paired", "not with paired-end reads"), ("SR", "paired", "not with paired-end reads"),
                                                ("XYZ", "paired", "must be one of"), ("isf", "paired", "must be one of")])
def test_cli_rejects_lib_type(lib_type, reads, why):
    r = ["-1", "a.fq", "-2", "b.fq"] if reads == "paired" else ["-r", "a.fq"]
    p = subprocess.run([sys.executable, "-m", "rapmap_amd", "quasimap", "-i", "nowhere", "--libType", lib_type, "-n"] + r,
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 2 and "--libType" in p.stderr and why in p.stderr
