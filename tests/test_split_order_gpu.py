"""A device-resident batch mapped in parts (map_device_split, qm_host.hip) whose parts finish in order: part p scans its counts from
the hits of the parts before it, writes its offsets straight into the caller's array, and writes its hits as soon as the caller's
result array holds base + own total records -- before the parts behind it have finished.  The array is replaced only at the
rendezvous of a call that outgrows it, and a part that wrote early writes again.

On ONE context, calls in a row -- a small batch (the first call: no array yet), larger ones (the array grows, also behind a part that
had written early), small ones (it does not) --, a batch whose first parts have no hits at all, and one -s call, in two and in three parts (QM_SPLIT_MIN=1000 splits small
batches): hits, offsets and counters of every call equal those of the unsplit call (QM_SPLIT=1) and the oracle's.  QM_DUO_PARTS and
QM_SPLIT_FIRST are read once per process: the test that varies them starts a fresh child process per value (this file run as a
script).  No error path is provoked here."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.gpu


def batches(reads1, reads2):
    """name -> (q1, o1, q2, o2) packed: small (1 200 pairs), mid (2 000: its first half fits the array that `small` left, the whole does not
    -- part 0 writes early, the array is replaced, part 0 writes again), large (all), small2 (1 300 others), nohits (1 900 pairs, the first
    1 300 of them random characters: no part 0 of two or of three parts has a hit)"""
    from util import pack
    n = len(reads1)
    assert n >= 4000, n
    rng = np.random.default_rng(17)
    junk = lambda: bytes(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 100)])
    sets = {"small": (reads1[:1200], reads2[:1200]), "mid": (reads1[:2000], reads2[:2000]), "large": (reads1, reads2),
            "small2": (reads1[1500:2800], reads2[1500:2800]),
            "nohits": ([junk() for _ in range(1300)] + reads1[3000:3600], [junk() for _ in range(1300)] + reads2[3000:3600])}
    return {k: pack(a) + pack(b) for k, (a, b) in sets.items()}


class Device:
    """the batches resident on the device, and calls of qm_map_device over them"""
    def __init__(self, mp, bat):
        import torch
        self.mp, self.t = mp, {}
        pad = np.zeros(8, np.uint8)                              # the device buffers extend past the last read (qmap_mi355.h)
        for k, (q1, o1, q2, o2) in bat.items():
            self.t[k] = [torch.from_numpy(x).cuda() for x in (np.concatenate([q1, pad]), o1, np.concatenate([q2, pad]), o2)]
        torch.cuda.synchronize()

    def map(self, name, opts=None):
        d = self.t[name]
        return self.mp.map_device(len(d[1]) - 1, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), 100, opts=opts, fetch=True)


SEQUENCE = ("small", "mid", "large", "small2", "nohits", "large", "small")


def key(r):
    """what two results are compared by: offsets, hit records (bytes), counters (by name)"""
    return np.asarray(r.hit_offsets), np.frombuffer(r.hits.tobytes(), dtype=np.uint8), np.array([v for _, v in sorted(r.counters.items())], dtype=np.int64)


def same(got, want, what):
    g = key(got)
    assert np.array_equal(g[0], want[0]), what + ": offsets"
    assert np.array_equal(g[1], want[1]), what + ": hit records"
    assert np.array_equal(g[2], want[2]), (what, got.counters, want[2])


def run_sequence(idx, bat, parts, want, sel_want=None, sel_opts=None):
    """a fresh context; the calls of SEQUENCE in `parts` parts, then (sel_want) one -s call; every result equals want[name] (a key())"""
    import mapping_harness as mh
    os.environ["QM_SPLIT_MIN"] = "1000"; os.environ["QM_SPLIT"] = str(parts)
    try:
        with mh.gpu_mapper(idx, debug=False) as (qi, mp):
            dev = Device(mp, bat)
            for i, name in enumerate(SEQUENCE):
                same(dev.map(name), want[name], "call %d (%s) in %d parts" % (i, name, parts))
            if sel_want is not None:
                same(dev.map("large", opts=sel_opts), sel_want, "-s in %d parts" % parts)
                same(dev.map("small"), want["small"], "after -s, in %d parts" % parts)
    finally:
        del os.environ["QM_SPLIT_MIN"]; del os.environ["QM_SPLIT"]


@pytest.fixture(scope="module")
def unsplit(synth_small, oracle_mod):
    """the batches, and every batch's result from the unsplit call, held against the oracle's"""
    import mapping_harness as mh
    import rapmap_amd as ra
    from conftest import load_oracle
    from util import assert_hits_equal
    bat = batches(synth_small["reads1"], synth_small["reads2"])
    ix, orc = load_oracle(synth_small["idx"])
    os.environ["QM_SPLIT"] = "1"
    try:
        with mh.gpu_mapper(synth_small["idx"], debug=False) as (qi, mp):
            dev = Device(mp, bat)
            want = {k: dev.map(k) for k in bat}
            sel = dev.map("large", opts=ra.default_opts(sel_aln=1))
    finally:
        del os.environ["QM_SPLIT"]
    for k, a in bat.items():
        res = orc.map_pairs(*a, nthreads=8)
        assert_hits_equal(res.hit_offsets, res.hits, want[k].hit_offsets, want[k].hits, "unsplit, " + k)
        assert res.counters == want[k].counters, (k, res.counters, want[k].counters)
    res = orc.map_pairs(*bat["large"], opts=oracle_mod.default_opts(selAln=1), nthreads=8)
    assert_hits_equal(res.hit_offsets, res.hits, sel.hit_offsets, sel.hits, "unsplit, -s")
    assert res.counters == sel.counters
    nh = want["nohits"].hit_offsets
    assert nh[1300] == 0 and nh[-1] > 0, "the junk pairs of `nohits` have hits, or the others none"
    hs, hm, hl = (int(want[k].hit_offsets[-1]) for k in ("small", "mid", "large"))
    cap = hs + 1 + hs // 8                                       # (the array a first call of `small` leaves: DevBuf::ensure with an eighth of slack)
    assert int(want["mid"].hit_offsets[1000]) + 1 <= cap < hm + 1, "`mid`: its first half should fit the array of `small`, the whole should not"
    assert hl + 1 > hm + 1 + hm // 8, "`large` does not outgrow the array of `mid`"
    return {"idx": synth_small["idx"], "bat": bat, "want": {k: key(r) for k, r in want.items()}, "sel": key(sel)}


@pytest.mark.parametrize("parts", [2, 3])
def test_calls_in_a_row(unsplit, parts):
    """first call, growth behind an early write, growth, no growth, a first part without hits, -s: in two and three parts on one context"""
    import rapmap_amd as ra
    run_sequence(unsplit["idx"], unsplit["bat"], parts, unsplit["want"], sel_want=unsplit["sel"], sel_opts=ra.default_opts(sel_aln=1))


@pytest.mark.parametrize("env", [{"QM_DUO_PARTS": "85"}, {"QM_SPLIT_FIRST": "30", "QM_DUO_PARTS": "0"}], ids=["pair_kernel_first", "uneven_lean_only"])
def test_other_part_layouts(unsplit, env, tmp_path):
    """the pair kernel on part 0 (the slower part first: the parts behind it wait for its total), and two uneven parts: a fresh process each"""
    f = str(tmp_path / "want.npz")
    arrays = {"%s_%s" % (k, j): x for k, a in unsplit["bat"].items() for j, x in zip(("q1", "o1", "q2", "o2"), a)}
    arrays.update({"%s_want%d" % (k, j): x for k, w in unsplit["want"].items() for j, x in enumerate(w)})
    np.savez(f, **arrays)
    e = dict(os.environ); e.update(env)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), unsplit["idx"], f], env=e, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "split order ok" in p.stdout


def _child(idx, path):
    """the calls of SEQUENCE in two parts under this process's QM_DUO_PARTS / QM_SPLIT_FIRST, against the results in `path`"""
    sys.path.insert(0, HERE); sys.path.insert(0, os.path.dirname(HERE))
    import torch
    torch.cuda.init()                                            # (torch's HIP runtime opens the device before the library's: conftest.lib_built)
    z = np.load(path)
    names = sorted({k.rsplit("_", 1)[0] for k in z.files})
    bat = {k: tuple(z["%s_%s" % (k, j)] for j in ("q1", "o1", "q2", "o2")) for k in names}
    want = {k: tuple(z["%s_want%d" % (k, j)] for j in range(3)) for k in names}
    run_sequence(idx, bat, 2, want)
    print("split order ok")


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
