"""Equivalence classes without a GPU: the device code (rapmap_amd/csrc/qm_eqc.inl) under the lane emulation, the file format, the CLI.

The emulation (tests/emu/qm_emu_eqc.cpp) runs one wavefront after the other and one lane after the other: it proves the LOGIC of the
label and insert stages -- grouping, ranking, sorting, repeats, keys, probing, claims, publishing, rebuilds -- not the atomics; what
contention does to them is the GPU tests' part (test_eq_classes_gpu.py)."""
import subprocess
import sys

import numpy as np
import pytest

import eqc_cases as ec
import part_cases as pc
from conftest import ROOT


@pytest.fixture(scope="module")
def emu():
    import emu_eqc
    emu_eqc._lib()
    return emu_eqc


@pytest.fixture(scope="module")
def crafted():
    L, w = ec.crafted_lists()
    off, tids = ec.csr(L)
    return L, w, off, tids


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("stride", [4, 32])
def test_emulated_crafted_lists(emu, crafted, weights, stride):
    L, w, off, tids = crafted
    ww = w if weights else None
    o, t, c, st = emu.run(off, tids, weights=ww, cap=1 << 14, pool_cap=1 << 16, stride=stride)
    d = ec.expected(L, ww)
    ec.assert_table((o, t, c), d, "crafted lists")
    assert int(c.sum()) == sum(d.values()) == sum((int(w[i]) if weights else 1) for i, x in enumerate(L) if len(x))
    assert st["growths"] == 0 and st["long_units"] == sum(1 for x in L if len(x) > 8)


def test_emulated_aggregation_changes_nothing(emu, crafted):
    L, w, off, tids = crafted
    a = emu.run(off, tids, weights=w, cap=1 << 14, pool_cap=1 << 16, aggregate=True)
    b = emu.run(off, tids, weights=w, cap=1 << 14, pool_cap=1 << 16, aggregate=False)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)


def test_emulated_forced_collisions(emu):
    L = ec.distinct_labels(500)
    off, tids = ec.csr(L)
    full = emu.run(off, tids, hash_bits=0, cap=2048, pool_cap=4096)
    few = emu.run(off, tids, hash_bits=4, cap=2048, pool_cap=4096)
    ec.assert_table(full[:3], ec.expected(L), "all key bits")
    ec.assert_table(few[:3], ec.expected(L), "four key bits")
    assert few[3]["collision_probes"] > 0


def test_emulated_growth_and_accumulation(emu, crafted):
    L = ec.distinct_labels(5000)
    off, tids = ec.csr(L)
    o, t, c, st = emu.run(off, tids, cap=16, pool_cap=64, folds=3)
    ec.assert_table((o, t, c), {k: 3 * v for k, v in ec.expected(L).items()}, "5 000 labels from a table of 16 slots, three folds")
    assert st["growths"] > 0
    L2, w, off2, tids2 = crafted                                    # labels of 1 100 and 2 500 tids into a pool of 64 words
    o, t, c, st = emu.run(off2, tids2, weights=w, cap=16, pool_cap=64)
    ec.assert_table((o, t, c), ec.expected(L2, w), "crafted lists from a table of 16 slots")
    assert st["growths"] > 0


@pytest.mark.parametrize("shape", sorted(pc.SHAPES))
def test_emulated_host_lists_in_parts(emu, shape):
    """qm_eqc_add_labels' driver, with weights, at MAX_UNITS lists and MAX_ITEMS tids to a part: the same table as in one part and as
    the restatement.  The table keeps no count of its folds; every part with a tid costs a round at least"""
    off = pc.offsets_of(shape)
    rng = np.random.default_rng(len(shape))
    n = len(off) - 1
    tids = None if shape == "null" else rng.integers(0, 4, int(off[-1])).astype(np.uint32)      # few transcripts: lists of different parts meet in a class
    w = rng.integers(1, 1 << 40, n).astype(np.uint64)
    lists = [[] if tids is None else tids[off[i]:off[i + 1]] for i in range(n)]
    small = emu.run(off, tids, weights=w, max_units=pc.MAX_UNITS, max_tids=pc.MAX_ITEMS)
    whole = emu.run(off, tids, weights=w, max_units=pc.ONE_PART, max_tids=pc.ONE_PART)
    ec.assert_table(small[:3], ec.expected(lists, w), shape); ec.assert_table(whole[:3], ec.expected(lists, w), shape + ", one part")
    for x, y in zip(small[:3], whole[:3]):
        assert x.tobytes() == y.tobytes()
    with_tids = sum(1 for a, b in pc.parts(off) if off[b] > off[a])
    assert small[3]["rounds"] >= with_tids and (small[3]["rounds"] == 0) == (with_tids == 0)
    if shape != "null" and off[0] == 0 and n:                        # the same lists folded where they lie (no host arrays, no parts)
        direct = emu.run(off, tids, weights=w)
        for x, y in zip(small[:3], direct[:3]):
            assert x.tobytes() == y.tobytes()


def test_emulated_decreasing_list_offsets(emu):
    with pytest.raises(emu.ArgError):
        emu.run(pc.decreasing(), np.arange(6, dtype=np.uint32), weights=np.ones(4, dtype=np.uint64), max_units=pc.MAX_UNITS, max_tids=pc.MAX_ITEMS)
    with pytest.raises(emu.ArgError):                                # tids that the offsets ask for are missing
        emu.run(np.array([0, 2], dtype=np.int64), None, max_units=pc.MAX_UNITS, max_tids=pc.MAX_ITEMS)


def test_write_parse_round_trip(tmp_path):
    import rapmap_amd as ra
    d = {(0,): 7, (0, 3): 1, (0, 3, ec.BIG): (1 << 40) + 1, (2,): 5, (1, 2, 3, 4, 5, 6, 7, 8, 9): 2}
    off, tids, cnt = ec.canonical(d)
    names = ["t%d" % i for i in range(12)] + ["a name|with.odd:chars"]
    p = str(tmp_path / "eq_classes.txt")
    ra.write_eq_classes(p, names, off, tids, cnt)
    lines = open(p).read().split("\n")
    assert lines[0] == "13" and lines[1] == "5" and lines[2:15] == names
    assert lines[15] == "1\t0\t7" and lines[16] == "2\t0\t3\t1" and lines[-1] == ""
    n2, o2, t2, c2 = ra.read_eq_classes(p)
    assert n2 == names
    ec.assert_table((o2, t2, c2), d, "round trip")


def test_cli_rejects_eq_classes_without_a_file():
    r = subprocess.run([sys.executable, "-m", "rapmap_amd", "quasimap", "-i", "nowhere", "-r", "reads.fq", "--eqClasses"],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 2 and "--eqClasses" in r.stderr and "expected one argument" in r.stderr
