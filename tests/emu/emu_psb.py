"""tests/emu/emu_psb.py -- ctypes face of the TEST-ONLY lane emulation of the positional bias model (libqm_emu_psb.so: the driver of
rapmap_amd/csrc/qm_psb_host.inl and the device code of qm_psb.inl compiled with -DQM_EMU by qm_emu_psb.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libqm_emu_psb.so")
_SRC = [os.path.join(_HERE, "qm_emu_psb.cpp")] + [os.path.join(_HERE, "../../rapmap_amd/csrc", f) for f in
                                                  ("qm_psb_host.inl", "qm_psb.inl", "qm_sqb_host.inl", "qm_sqb.inl", "qm_gcb.inl", "qm_tally_host.inl", "qm_sweep.h",
                                                   "qm_exec.h", "qm_grid.h", "qm_wave.h")] + [os.path.join(_HERE, "../../include/qmap_mi355.h")]
BINS, SHAPE, C_WORDS = 200, (2, 5, 20), 8
STATS = ("units", "used", "unmapped", "multi", "not_paired", "same_strand", "out_of_range", "overhang", "max_len", "folds", "last_fold_us",
         "last_expect_us", "last_efflen_us")                         # the order of QM_PSB_STAT_*
PART_UNITS, PART_HITS = 1 << 22, 1 << 21                             # a part of host arrays, as qm_psb_add_hits cuts them


class ArgError(RuntimeError):
    """what the device reports as QM_E_ARG (-1)"""


def build():
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused", "-ffp-contract=off", "-o", _LIB, _SRC[0]])


_cached = None


def _lib():
    global _cached
    if _cached is not None:
        return _cached
    if not os.path.exists(_LIB) or any(os.path.getmtime(_LIB) < os.path.getmtime(s) for s in _SRC):
        build()
    lib = C.CDLL(_LIB)
    lib.qe_psb_create.restype = C.c_void_p
    for f in (lib.qe_psb_obs_grid, lib.qe_psb_exp_grid, lib.qe_psb_tile_grid, lib.qe_psb_add_hits, lib.qe_psb_add_counts, lib.qe_psb_clear, lib.qe_psb_fetch,
              lib.qe_psb_stat, lib.qe_psb_expect, lib.qe_psb_eff_lens, lib.qe_psb_position, lib.qe_psb_weights, lib.qe_psb_ratios):
        f.restype = C.c_int
    lib.qe_psb_destroy.restype = None
    _cached = lib
    return lib


def _check(rc, what):
    if rc == -1:
        raise ArgError("%s -1" % what)
    if rc:
        raise RuntimeError("%s failed (%d)" % (what, rc))


def _p(a):
    return C.c_void_p(a.ctypes.data if a.size else None)


def weights(alpha, lens, counts):
    """the emulation build's sqb_weights: (q uint64[T], k)"""
    c = np.ascontiguousarray(counts, dtype=np.uint64); ln = np.ascontiguousarray(lens, dtype=np.uint32); a = np.ascontiguousarray(alpha, dtype=np.float64)
    q = np.zeros(ln.size, dtype=np.uint64); k = C.c_int32(0)
    _check(_lib().qe_psb_weights(C.c_int(c.size - 1), _p(c), C.c_longlong(ln.size), _p(ln), _p(a), _p(q), C.byref(k)), "qe_psb_weights")
    return q, int(k.value)


def ratios(obs, ex):
    o = np.ascontiguousarray(obs, dtype=np.uint64).ravel(); e = np.ascontiguousarray(ex, dtype=np.uint64).ravel()
    assert o.size == BINS == e.size
    R = np.zeros(BINS, dtype=np.float64)
    _check(_lib().qe_psb_ratios(_p(o), _p(e), _p(R)), "qe_psb_ratios")
    return R.reshape(SHAPE)


class EmuPsb:
    """the emulated driver behind the interface of rapmap_amd.PosBias (what tests/psb_cases.py drives), over transcripts of its own:
    offsets and lens; max_units / max_hits: the caps of a part of add_hits' arrays (the library's by default)"""

    def __init__(self, offsets, lens, max_len=1000, max_blocks=0, max_units=PART_UNITS, max_hits=PART_HITS):
        self.max_len, self.max_blocks, self.max_units, self.max_hits = int(max_len), int(max_blocks), int(max_units), int(max_hits)
        off = np.ascontiguousarray(offsets, dtype=np.uint32); ln = np.ascontiguousarray(lens, dtype=np.int32)
        self.n_txps = int(off.size)
        n = int(off[-1]) + int(ln[-1]) + 1 if off.size else 0
        self._h = _lib().qe_psb_create(C.c_longlong(n), C.c_longlong(off.size), C.c_void_p(off.ctypes.data), C.c_void_p(ln.ctypes.data), C.c_int(self.max_len),
                                       C.c_int(self.max_blocks))
        if not self._h:
            raise ArgError("max_len -1")

    def clear(self):
        _check(_lib().qe_psb_clear(C.c_void_p(self._h)), "qe_psb_clear")

    def add_hits(self, hit_offsets, hits):
        off = np.ascontiguousarray(hit_offsets, dtype=np.int64)
        n = len(off) - 1
        raw = None
        if hits is not None and len(hits):
            raw = np.ascontiguousarray(hits).view(np.uint8)
            assert hits.dtype.itemsize == 32 and int(off[-1]) <= len(hits)
        elif n > 0:
            assert int(off[-1]) == int(off[0])
        _check(_lib().qe_psb_add_hits(C.c_void_p(self._h), C.c_longlong(n), C.c_void_p(off.ctypes.data), C.c_void_p(raw.ctypes.data if raw is not None else None),
                                      C.c_longlong(self.max_units), C.c_longlong(self.max_hits)), "qe_psb_add_hits")

    def add_counts(self, obs):
        c = np.ascontiguousarray(obs, dtype=np.uint64).ravel()
        if c.size != BINS:
            raise ArgError("counts -1")
        _check(_lib().qe_psb_add_counts(C.c_void_p(self._h), _p(c)), "qe_psb_add_counts")

    def counts(self):
        bins = np.zeros(BINS, dtype=np.uint64); ctr = np.zeros(C_WORDS, dtype=np.uint64)
        _check(_lib().qe_psb_fetch(C.c_void_p(self._h), _p(bins), _p(ctr)), "qe_psb_fetch")
        return bins.reshape(SHAPE)

    def stat(self):
        v = C.c_int64(0); d = {}
        for which, k in enumerate(STATS):
            _check(_lib().qe_psb_stat(C.c_void_p(self._h), C.c_int(which), C.byref(v)), "qe_psb_stat")
            d[k] = int(v.value)
        return d

    def expect(self, counts, n_txps, q):
        c = np.ascontiguousarray(counts, dtype=np.uint64); q = np.ascontiguousarray(q, dtype=np.uint64)
        assert c.size == self.max_len + 1
        ex = np.zeros(BINS, dtype=np.uint64)
        rc = _lib().qe_psb_expect(C.c_void_p(self._h), _p(c), C.c_longlong(int(n_txps)), _p(q), _p(ex))
        if rc == -4:
            raise RuntimeError("qe_psb_expect -4")
        _check(rc, "qe_psb_expect")
        return ex.reshape(SHAPE)

    def eff_lens(self, counts, n_txps, R):
        c = np.ascontiguousarray(counts, dtype=np.uint64); R = np.ascontiguousarray(R, dtype=np.float64).ravel()
        assert c.size == self.max_len + 1 and R.size == BINS
        eff = np.zeros(int(n_txps), dtype=np.float64)
        _check(_lib().qe_psb_eff_lens(C.c_void_p(self._h), _p(c), C.c_longlong(int(n_txps)), _p(R), _p(eff)), "qe_psb_eff_lens")
        return eff

    def position(self, tids, positions):
        t = np.ascontiguousarray(tids, dtype=np.uint32); p = np.ascontiguousarray(positions, dtype=np.int32)
        out = np.zeros((t.size, 2), dtype=np.int32)
        _check(_lib().qe_psb_position(C.c_void_p(self._h), C.c_longlong(t.size), _p(t), _p(p), _p(out)), "qe_psb_position")
        return out

    def close(self):
        if self._h:
            _lib().qe_psb_destroy(C.c_void_p(self._h)); self._h = None
