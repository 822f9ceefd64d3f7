"""The grid arithmetic of the launch layer (rapmap_amd/csrc/qm_grid.h: no HIP, compiled here with g++) against expectations worked out by
hand from the formulas the launchers carried before they shared it:

    blocks = max(1, min((work + 3) / 4, num_cu * resident_per_cu * oversub))

for num_cu = 256 (a whole MI355X).  Every expectation is a literal; nothing is recomputed from the code under test."""
import os
import subprocess

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emu", "qm_grid_check.cpp")
_KNOBS = ("QM_GRID_OVERSUB", "QM_GRID_OVERSUB_PH", "QM_BLOCKS_PER_CU", "QM_DUO_OVERSUB")


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grid") / "qm_grid_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, _SRC])

    def run(questions, **knobs):
        env = {k: v for k, v in os.environ.items() if k not in _KNOBS}
        env.update(knobs)
        out = subprocess.check_output([exe] + list(questions), env=env, text=True)
        return [int(x) for x in out.split()]
    return run


def test_small_work_gets_one_block_per_four_units(ask):
    # 0, 1, 4, 5 reads at resident 8, oversub 4: never fewer than one block, four waves to a block
    assert ask(["blocks:0,256,8,4", "blocks:1,256,8,4", "blocks:4,256,8,4", "blocks:5,256,8,4"]) == [1, 1, 1, 2]


@pytest.mark.parametrize("oversub,cap", [(1, 2048), (4, 8192), (12, 24576)])      # cap = 256 CUs x 8 resident x oversub
def test_cap_edges(ask, oversub, cap):
    tail = ",256,8,%d" % oversub
    # work for exactly cap blocks, for one block less, for one unit more (cap + 1 blocks wanted), and the last unit that still fits
    got = ask(["blocks:%d%s" % (w, tail) for w in (4 * cap, 4 * cap - 4, 4 * cap + 1, 4 * cap - 3)])
    assert got == [cap, cap - 1, cap, cap]
    # the same in blocks (the launchers that are handed the caller's grid)
    assert ask(["clamp:%d%s" % (b, tail) for b in (cap, cap - 1, cap + 1, 0)]) == [cap, cap - 1, cap, 1]


def test_literal_caps(ask):
    # the three caps above once more as plain numbers, so that the parametrised test's arithmetic is not the only witness
    assert ask(["blocks:1000000,256,8,1", "blocks:1000000,256,8,4", "blocks:1000000,256,8,12"]) == [2048, 8192, 24576]
    assert ask(["blocks:8192,256,8,1", "blocks:8188,256,8,1", "blocks:8193,256,8,1"]) == [2048, 2047, 2048]
    assert ask(["blocks:32768,256,8,4", "blocks:32764,256,8,4", "blocks:32769,256,8,4"]) == [8192, 8191, 8192]
    assert ask(["blocks:98304,256,8,12", "blocks:98300,256,8,12", "blocks:98305,256,8,12"]) == [24576, 24575, 24576]
    # a kernel whose occupancy is 2 blocks per CU (the list kernels' fallback), no oversubscription: 512 blocks
    assert ask(["clamp:8192,256,2,1", "clamp:511,256,2,1"]) == [512, 511]


def test_resident_grid(ask):
    # oversub 1 at the nominal 8 blocks per CU, whatever the knobs say
    q = ["resident:0,256", "resident:5,256", "resident:8188,256", "resident:8192,256", "resident:8193,256", "resident:20000000,256"]
    assert ask(q) == [1, 2, 2047, 2048, 2048, 2048]
    assert ask(q, QM_GRID_OVERSUB="2", QM_GRID_OVERSUB_PH="6") == [1, 2, 2047, 2048, 2048, 2048]


def test_sweep_grid(ask):
    # the fragment-length fold and the library-type sweep: one lane per unit or hit, 256 to a block, 8 resident per CU, no
    # oversubscription, then the caller's max_blocks (the last argument; 0: none).  The values test_fld.py and test_lib_format.py hold
    # the emulated grids to, asked of the shared function
    q = ["sweep:70001,256,8,1", "sweep:70001,256,8,2", "sweep:70001,256,8,0", "sweep:10000000,256,8,0", "sweep:1,256,8,0", "sweep:257,256,8,0"]
    assert ask(q) == [1, 2, 274, 2048, 1, 2]
    # no lanes: one block; exactly one block's lanes and one more; the cap's edges; a cap above what the work wants; no compute units known
    assert ask(["sweep:0,256,8,0", "sweep:256,256,8,0", "sweep:524288,256,8,0", "sweep:524032,256,8,0", "sweep:524289,256,8,0"]) == [1, 1, 2048, 2047, 2048]
    assert ask(["sweep:70001,256,8,274", "sweep:70001,256,8,273", "sweep:70001,256,8,5000", "sweep:1000,0,8,0", "sweep:10000,0,8,0"]) == [274, 273, 274, 4, 8]
    assert ask(q, QM_GRID_OVERSUB="2", QM_GRID_OVERSUB_PH="6") == [1, 2, 274, 2048, 1, 2]


def test_lean_and_pair_iterations(ask):
    # narrow lean kernel: two reads per trip, (nreads + 1) >> 1; wide: one read per trip; pair kernel: nreads >> 1
    assert ask(["lean:0,0", "lean:1,0", "lean:2,0", "lean:3,0", "lean:7,0", "lean:20000000,0"]) == [0, 1, 1, 2, 4, 10000000]
    assert ask(["lean:0,1", "lean:1,1", "lean:7,1", "lean:20000000,1"]) == [0, 1, 7, 20000000]
    assert ask(["pair:0", "pair:2", "pair:8", "pair:20000000"]) == [0, 1, 4, 10000000]
    # ... and the grids they lead to: 10 reads are 5 trips, two blocks; 10 M pairs at resident 8 and twice the default oversubscription
    assert ask(["blocks:5,256,8,8", "blocks:10000000,256,8,8", "blocks:10000000,256,8,1"]) == [2, 16384, 2048]


def test_oversubscription_knobs(ask):
    q = ["oversub", "oversub_ph", "map:100000,256,0", "map:100000,256,1", "map:20000000,256,0", "map:20000000,256,1"]
    # defaults: 4 and 12; 100 000 reads want 25 000 blocks
    assert ask(q) == [4, 12, 8192, 24576, 8192, 24576]
    # QM_GRID_OVERSUB alone also sets the compact -p kernels' factor
    assert ask(q, QM_GRID_OVERSUB="2") == [2, 2, 4096, 4096, 4096, 4096]
    assert ask(q, QM_GRID_OVERSUB_PH="6") == [4, 6, 8192, 12288, 8192, 12288]
    assert ask(q, QM_GRID_OVERSUB="2", QM_GRID_OVERSUB_PH="16") == [2, 16, 4096, 25000, 4096, 32768]
    # out of range (1 .. 16): as if unset -- but a set QM_GRID_OVERSUB still decides the -p factor's fallback
    assert ask(q, QM_GRID_OVERSUB="17") == [4, 4, 8192, 8192, 8192, 8192]
    assert ask(q, QM_GRID_OVERSUB="0", QM_GRID_OVERSUB_PH="0") == [4, 4, 8192, 8192, 8192, 8192]
    assert ask(q, QM_GRID_OVERSUB_PH="17") == [4, 12, 8192, 24576, 8192, 24576]
