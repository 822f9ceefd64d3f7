"""tests/emu/emu_runs.py -- ctypes face of tests/emu/qm_emu_runs.cpp (TEST-ONLY): a paired batch through one headline kernel's wave driver
under a chosen schedule, and on to hit records as the library goes on behind that kernel.  The index arrays are emu.Emu's."""
import ctypes as C
import os
import subprocess

import numpy as np

import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libqm_emu_runs.so")
_SRC = [os.path.join(_HERE, "qm_emu_runs.cpp"), os.path.join(_HERE, "../../rapmap_amd/csrc/qm_grid.h")] + emu._SRC
KERNELS = {"pair": 0, "lean": 1}


def _lib():
    if not os.path.exists(_LIB) or any(os.path.getmtime(_LIB) < os.path.getmtime(s) for s in _SRC):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused", "-o", _LIB, _SRC[0]])
    return C.CDLL(_LIB)


def map_runs(em, kernel, nw, run, seq1, off1, seq2, off2, opts=None):
    """em: an emu.Emu of a dense index; kernel: "pair" or "lean"; nw waves, runs of `run` pairs -> a result as emu.Emu.map gives it
    (hit_offsets, hits, counters, status) with .left (reads the kernel left to the general one) and .merged (pairs merged in the wavefront)"""
    assert em.ph is None, "a dense index"
    lib = _lib()
    opts = opts or emu.default_opts()
    nunits = len(off1) - 1
    pad = np.zeros(8, dtype=np.uint8)                            # reads are fetched four characters at a time
    seq1 = np.concatenate([np.asarray(seq1, dtype=np.uint8), pad]); off1 = np.ascontiguousarray(off1, dtype=np.int64)
    seq2 = np.concatenate([np.asarray(seq2, dtype=np.uint8), pad]); off2 = np.ascontiguousarray(off2, dtype=np.int64)
    ho = np.zeros(nunits + 1, dtype=np.int64)
    ctr = np.zeros(6, dtype=np.uint64)
    stats = np.zeros(3, dtype=np.int64)
    hp = C.c_void_p()
    rc = lib.qe_runs_map(C.c_int(em.ix.k), C.c_void_p(em.text.ctypes.data), C.c_int64(em.n), C.c_void_p(em.SA.ctypes.data), C.c_int64(em.SA.size),
                         C.c_void_p(em.sainfo.ctypes.data), C.c_void_p(em.slots.ctypes.data), C.c_uint64(em.cap - 1), C.byref(opts), C.c_int64(nunits),
                         C.c_void_p(seq1.ctypes.data), C.c_void_p(off1.ctypes.data), C.c_void_p(seq2.ctypes.data), C.c_void_p(off2.ctypes.data),
                         C.c_int(KERNELS[kernel]), C.c_int(nw), C.c_int(run), C.c_void_p(ho.ctypes.data), C.byref(hp), C.c_void_p(ctr.ctypes.data),
                         C.c_void_p(stats.ctypes.data))
    assert rc == 0, rc
    tot = int(ho[-1])
    hits = np.ctypeslib.as_array(C.cast(hp, C.POINTER(C.c_uint8)), shape=((tot + 1) * 32,))[: tot * 32].copy().view(emu.HIT_DTYPE)
    lib.qe_free(hp)

    class R:
        pass
    r = R()
    r.hit_offsets, r.hits, r.status, r.left, r.merged = ho, hits, int(stats[2]), int(stats[0]), int(stats[1])
    r.counters = dict(zip(["peHits", "seHits", "totHits", "numReads", "tooManyHits", "mappedUnits"], [int(x) for x in ctr]))
    return r
