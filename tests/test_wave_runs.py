"""The run schedule of the two headline kernels (rapmap_amd/csrc/qm_grid.h: no HIP, compiled here with g++ into tests/emu/qm_runs_check.cpp):
wave gw of nw takes the runs gw, gw + nw, .. of R = 1 << rs neighbouring trips and maps each run's trips in order.

    trip t of wave gw = (((t >> rs) * nw + gw) << rs) + (t & (R - 1)),   through when that is not below the number of trips

The wave drivers walk it with run_next / run_ends; the check program walks every wave of a grid the same way and counts.  R shrinks until
the batch has at least as many runs as waves can be resident (num_cu x 32: 8 192 on a whole MI355X).  Every expectation is a literal."""
import os
import subprocess

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "emu", "qm_runs_check.cpp")
_KNOBS = ("QM_GRID_OVERSUB", "QM_GRID_OVERSUB_PH", "QM_BLOCKS_PER_CU", "QM_DUO_OVERSUB", "QM_WAVE_RUN")


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("runs") / "qm_runs_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, _SRC])

    def run(questions, **knobs):
        env = {k: v for k, v in os.environ.items() if k not in _KNOBS}
        env.update(knobs)
        out = subprocess.check_output([exe] + list(questions), env=env, text=True)
        return [[int(x) for x in line.split()] for line in out.splitlines()]
    return run


# trips: 0, 1, R - 1, R, R + 1, 2 R + 3, 1 000 003, by run shift
TRIPS = {0: (0, 1, 0, 1, 2, 5, 1000003), 1: (0, 1, 1, 2, 3, 7, 1000003), 3: (0, 1, 7, 8, 9, 19, 1000003)}


@pytest.mark.parametrize("nw", [1, 3, 64, 65536])
@pytest.mark.parametrize("rs", [0, 1, 3])
def test_every_trip_once_and_in_order(ask, rs, nw):
    """every trip is visited exactly once; inside a run a wave steps to the neighbour, behind it to the start of a later run; run_trip
    names the same trips as the walk"""
    got = ask(["walk:%d,%d,%d" % (n, nw, rs) for n in TRIPS[rs]])
    assert [g[:4] for g in got] == [[n, 0, 0, 0] for n in TRIPS[rs]], got


def test_trips_per_wave(ask):
    # 1 000 003 trips in runs of 8 are 125 001 runs, the last of three trips; over 64 waves that is 1 953 runs each and nine left: waves 0-7
    # make 1 954 full runs (15 632 trips), wave 8 makes 1 953 and the short one (15 627), the others 1 953 (15 624)
    assert ask(["walk:1000003,64,3"]) == [[1000003, 0, 0, 0, 15632, 15624]]
    assert ask(["count:1000003,3", "count:1000003,0", "count:8,3", "count:9,3", "count:0,3"]) == [[125001], [1000003], [1], [2], [0]]
    # R = 1 is the strided order: 1 000 003 trips over 64 waves, 15 626 for waves 0-2 and 15 625 for the others
    assert ask(["walk:1000003,64,0"]) == [[1000003, 0, 0, 0, 15626, 15625]]
    # more waves than runs: the others find nothing
    assert ask(["walk:19,65536,3", "walk:7,3,3"]) == [[19, 0, 0, 0, 8, 0], [7, 0, 0, 0, 7, 0]]


def test_the_trips_of_a_wave(ask):
    # 19 trips, three waves, runs of eight: two full runs and a short one
    assert ask(["wave:19,3,3,%d" % g for g in range(3)]) == [list(range(0, 8)), list(range(8, 16)), [16, 17, 18]]
    # 11 trips, three waves, runs of two: every wave makes two runs, the last one is short
    assert ask(["wave:11,3,1,%d" % g for g in range(3)]) == [[0, 1, 6, 7], [2, 3, 8, 9], [4, 5, 10]]
    # runs of one: gw, gw + nw, ..
    assert ask(["wave:7,3,0,%d" % g for g in range(3)]) == [[0, 3, 6], [1, 4], [2, 5]]
    # a batch shorter than a run belongs to wave 0
    assert ask(["wave:5,2,3,0", "wave:5,2,3,1"]) == [[0, 1, 2, 3, 4], []]
    # trip t of a wave, directly: wave 2 of 5, runs of eight: its second run starts at (1 * 5 + 2) * 8
    assert ask(["trip:0,2,5,3", "trip:7,2,5,3", "trip:8,2,5,3", "trip:17,2,5,3", "trip:3,2,5,0"]) == [[16], [23], [56], [97], [17]]
    # the run `ahead` runs of the wave behind trip 21's (run 2, of 5 waves, 1 000 trips): runs 7 and 12 start at 56 and 96; none: the trip count
    assert ask(["ahead:21,1000,5,1", "ahead:21,1000,5,2", "ahead:21,60,5,2", "ahead:21,57,5,1", "ahead:21,56,5,1"]) == [[56], [96], [60], [56], [56]]


def test_run_length_shrinks_to_keep_the_device_full(ask):
    # 8 192 waves can be resident on 256 compute units; runs of 8 are kept while the batch has 8 192 runs of them
    q = ["shift:%d,8192,8" % n for n in (10000000, 65536, 65529, 65528, 32768, 32765, 32764, 16384, 16383, 16382, 10000, 1, 0)]
    assert ask(q) == [[3], [3], [3], [2], [2], [2], [1], [1], [1], [0], [0], [0], [0]]
    # the batches of the compat face, 10 000 to 140 000 pairs: runs of 1, 2 (20 000), 4 (50 000) and 8 (100 000, 140 000)
    assert ask(["shift:%d,8192,8" % n for n in (10000, 20000, 50000, 100000, 140000)]) == [[0], [1], [2], [3], [3]]
    # what was asked for is the ceiling; beyond eight: eight (the kernels' staging rows hold the offsets of eight trips)
    assert ask(["shift:10000000,8192,%d" % w for w in (1, 2, 4, 8, 16)]) == [[0], [1], [2], [3], [3]]
    # a smaller device keeps longer runs: 32 compute units, 1 024 resident waves
    assert ask(["shift:10000,1024,8", "shift:8185,1024,8", "shift:8184,1024,8", "shift:4000,1024,8"]) == [[3], [3], [2], [1]]


def test_knob_and_grid(ask):
    assert ask(["wave_run"]) == [[8]]
    assert [ask(["wave_run"], QM_WAVE_RUN=v) for v in ("1", "2", "4", "8")] == [[[1]], [[2]], [[4]], [[8]]]
    assert [ask(["wave_run"], QM_WAVE_RUN=v) for v in ("0", "3", "16", "x")] == [[[8]]] * 4            # anything else: the default
    # blocks of one, two and four waves for 16 384 four-wave units
    assert ask(["wave_blocks:16384,1", "wave_blocks:16384,2", "wave_blocks:16384,4"]) == [[65536], [32768], [16384]]
    # (waves, run shift) of a launch at 256 CUs, eight four-wave units resident per CU, oversubscribed eight times: 10 M pairs; 19 pairs
    # (five units: 20 waves); 100 000 pairs; and under QM_WAVE_RUN=1
    q = ["grid:10000000,256,8,8", "grid:19,256,8,8", "grid:100000,256,8,8", "grid:30000,256,8,8"]
    assert ask(q) == [[65536, 3], [20, 0], [65536, 3], [30000, 1]]
    assert ask(q, QM_WAVE_RUN="1") == [[65536, 0], [20, 0], [65536, 0], [30000, 0]]
    # QM_BLOCKS_PER_CU=1 with no oversubscription, as the launchers see it (one unit per CU): 1 024 waves, and runs of 8 from 8 192 pairs on
    assert ask(["grid:24000,256,1,1", "grid:8192,256,1,1", "grid:8184,256,1,1"]) == [[1024, 3], [1024, 3], [1024, 2]]
