"""Host arrays that go to an estimation object in parts (qx::feed of rapmap_amd/csrc/qm_exec.h, behind qm_fld_add_hits, qm_lib_add_hits,
qm_lib_compact_hits and qm_eqc_add_labels): the shapes at which the cut can go wrong, and the rule of the cut restated.  The library's
caps are constants no CPU test reaches; the emulation faces take them as arguments, and these shapes are fed at MAX_UNITS units and
MAX_ITEMS items (hits, tids) to a part.  test_fld.py, test_lib_format.py and test_eq_classes.py hold the result to the same input fed in
one part and to their numpy restatement, and the number of folds / sweeps to len(parts(...))."""
import functools

import numpy as np

MAX_UNITS, MAX_ITEMS = 3, 5
ONE_PART = 1 << 40                                                   # caps no input here reaches


def parts(offsets, max_units=MAX_UNITS, max_items=MAX_ITEMS):
    """[(u0, u1)]: a part takes one unit and is extended while it has fewer than max_units and the next unit still fits"""
    off = [int(x) for x in offsets]; out = []; u0 = 0
    while u0 < len(off) - 1:
        u1 = u0 + 1
        while u1 < len(off) - 1 and u1 - u0 < max_units and off[u1 + 1] - off[u0] <= max_items:
            u1 += 1
        out.append((u0, u1)); u0 = u1
    return out


# name -> (unit sizes, offsets[0], the parts' sizes in items as worked out by hand); "null": all units empty and no item array at all
SHAPES = {
    "no units": ([], 0, []),
    "one unit": ([2], 0, [2]),
    "a unit beyond the cap travels alone": ([1, 7, 1], 0, [1, 7, 1]),
    "a part of exactly the cap": ([2, 3, 1, 1], 0, [5, 2]),
    "a unit of the cap plus one": ([6], 0, [6]),
    "the cap plus one is cut": ([2, 4, 1], 0, [2, 5]),
    "more empty units than a part takes": ([0] * 7 + [1], 0, [0, 0, 1]),
    "offsets that do not start at 0": ([1, 2, 3, 0, 4, 1], 11, [3, 3, 5]),
    "null": ([0] * 4, 0, [0, 0]),
}


def offsets_of(name):
    sizes, base, by_hand = SHAPES[name]
    off = np.full(len(sizes) + 1, base, dtype=np.int64)
    if sizes:
        off[1:] += np.cumsum(np.asarray(sizes, dtype=np.int64))
    p = parts(off)
    assert [int(off[b] - off[a]) for a, b in p] == by_hand, name     # the restated rule gives the parts worked out by hand
    assert all(0 < b - a <= MAX_UNITS for a, b in p) and [a for a, _ in p] == ([0] + [b for _, b in p][:-1] if p else [])
    return off


def decreasing():
    """offsets that decrease at unit 2 (after two units that would make a part of their own)"""
    return np.array([0, 2, 5, 4, 6], dtype=np.int64)


LIB_PART_UNITS, LIB_PART_HITS = 1 << 22, 1 << 21                     # the library's caps for arrays of hits (qm_fld_add_hits, qm_lib_add_hits)


@functools.lru_cache(maxsize=1)
def big_batch():
    """(hit_offsets, hits): (1 << 21) + 65 hits over about 300 000 units -- the smallest input that does not fit into one part of the
    library's; units of lib_cases.UNIT_SIZES hits, records of lib_cases.records with fragment lengths on both sides of 1000.  Shared by
    the device tests that feed it; never changed."""
    import lib_cases as lc
    rng = np.random.default_rng(77)
    total = LIB_PART_HITS + 65
    sizes = rng.choice(np.asarray(lc.UNIT_SIZES), 320000, p=[.2, .35, .2, .1, .1, .02, .02, .01])
    cum = np.cumsum(sizes)
    n = int(np.searchsorted(cum, total))                             # the first unit that reaches the total is cut to what is left
    sizes = sizes[: n + 1].copy(); sizes[n] -= cum[n] - total
    off = lc.offsets_of(sizes)
    h = lc.records(lc.random_codes(total, rng), rng)
    h["frag_len"] = rng.integers(0, 1200, total)
    assert int(off[-1]) == total and 250000 < n < 320000 and len(parts(off, LIB_PART_UNITS, LIB_PART_HITS)) == 2
    off.setflags(write=False); h.setflags(write=False)
    return off, h
