"""tests/emu/emu_gcb.py -- ctypes face of the TEST-ONLY lane emulation of the fragment GC bias model (libqm_emu_gcb.so: the driver of
rapmap_amd/csrc/qm_gcb_host.inl and the device code of qm_gcb.inl compiled with -DQM_EMU by qm_emu_gcb.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libqm_emu_gcb.so")
_SRC = [os.path.join(_HERE, "qm_emu_gcb.cpp")] + [os.path.join(_HERE, "../../rapmap_amd/csrc", f) for f in
                                                  ("qm_gcb_host.inl", "qm_gcb.inl", "qm_tally_host.inl", "qm_sweep.h", "qm_exec.h", "qm_grid.h", "qm_wave.h")] + \
       [os.path.join(_HERE, "../../include/qmap_mi355.h")]
BINS, SLAB, C_WORDS = 25, 32, 8
STATS = ("units", "used", "unmapped", "multi", "not_paired", "same_strand", "out_of_range", "overhang", "max_len", "folds", "last_fold_us",
         "last_expect_us", "rank_build_us")                          # the order of QM_GCB_STAT_*
PART_UNITS, PART_HITS = 1 << 22, 1 << 21                             # a part of host arrays, as qm_gcb_add_hits cuts them


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
    lib.qe_gcb_create.restype = C.c_void_p
    lib.qe_gcb_rank.restype = C.c_longlong
    for f in (lib.qe_gcb_obs_grid, lib.qe_gcb_add_hits, lib.qe_gcb_add_counts, lib.qe_gcb_clear, lib.qe_gcb_fetch, lib.qe_gcb_stat, lib.qe_gcb_expect,
              lib.qe_gcb_window_gc):
        f.restype = C.c_int
    lib.qe_gcb_destroy.restype = None
    _cached = lib
    return lib


def _check(rc, what):
    if rc == -1:
        raise ArgError("%s -1" % what)
    if rc:
        raise RuntimeError("%s failed (%d)" % (what, rc))


class EmuGcb:
    """the emulated driver behind the interface of rapmap_amd.GCBias (what tests/gcb_cases.py drives), over a text of its own: text
    uint8[n], offsets and lens of its transcripts; max_units / max_hits: the caps of a part of add_hits' arrays (the library's by default)"""

    def __init__(self, text, offsets, lens, max_len=1000, max_blocks=0, max_units=PART_UNITS, max_hits=PART_HITS):
        self.max_len, self.max_blocks, self.max_units, self.max_hits = int(max_len), int(max_blocks), int(max_units), int(max_hits)
        text = np.ascontiguousarray(text, dtype=np.uint8); off = np.ascontiguousarray(offsets, dtype=np.uint32); ln = np.ascontiguousarray(lens, dtype=np.int32)
        self.n, self.n_txps = int(text.size), int(off.size)
        self._h = _lib().qe_gcb_create(C.c_void_p(text.ctypes.data), C.c_longlong(text.size), C.c_longlong(off.size), C.c_void_p(off.ctypes.data),
                                       C.c_void_p(ln.ctypes.data), C.c_int(self.max_len), C.c_int(self.max_blocks))
        if not self._h:
            raise ArgError("max_len -1")

    def rank_structure(self):
        """(mask uint64[blocks], rank uint32[blocks]) as the driver built them"""
        nb = _lib().qe_gcb_rank(C.c_void_p(self._h), None, None)
        m = np.zeros(nb, dtype=np.uint64); r = np.zeros(nb, dtype=np.uint32)
        _lib().qe_gcb_rank(C.c_void_p(self._h), C.c_void_p(m.ctypes.data), C.c_void_p(r.ctypes.data))
        return m, r

    def clear(self):
        _check(_lib().qe_gcb_clear(C.c_void_p(self._h)), "qe_gcb_clear")

    def add_hits(self, hit_offsets, hits):
        off = np.ascontiguousarray(hit_offsets, dtype=np.int64)
        n = len(off) - 1
        raw = None
        if hits is not None and len(hits):
            raw = np.ascontiguousarray(hits).view(np.uint8)
            assert hits.dtype.itemsize == 32 and int(off[-1]) <= len(hits)
        elif n > 0:
            assert int(off[-1]) == int(off[0])
        _check(_lib().qe_gcb_add_hits(C.c_void_p(self._h), C.c_longlong(n), C.c_void_p(off.ctypes.data), C.c_void_p(raw.ctypes.data if raw is not None else None),
                                      C.c_longlong(self.max_units), C.c_longlong(self.max_hits)), "qe_gcb_add_hits")

    def add_counts(self, obs):
        c = np.ascontiguousarray(obs, dtype=np.uint64)
        if c.size != BINS:
            raise ArgError("counts -1")
        _check(_lib().qe_gcb_add_counts(C.c_void_p(self._h), C.c_void_p(c.ctypes.data)), "qe_gcb_add_counts")

    def counts(self):
        bins = np.zeros(SLAB, dtype=np.uint64); ctr = np.zeros(C_WORDS, dtype=np.uint64)
        _check(_lib().qe_gcb_fetch(C.c_void_p(self._h), C.c_void_p(bins.ctypes.data), C.c_void_p(ctr.ctypes.data)), "qe_gcb_fetch")
        assert not bins[BINS:].any() and not ctr[7:].any()            # nothing lands beyond the last bin or counter
        return bins[:BINS].copy()

    def stat(self):
        v = C.c_int64(0); d = {}
        for which, k in enumerate(STATS):
            _check(_lib().qe_gcb_stat(C.c_void_p(self._h), C.c_int(which), C.byref(v)), "qe_gcb_stat")
            d[k] = int(v.value)
        return d

    def expect(self, counts, n_txps):
        c = np.ascontiguousarray(counts, dtype=np.uint64)
        assert c.size == self.max_len + 1
        H = np.zeros((int(n_txps), BINS), dtype=np.uint64)
        rc = _lib().qe_gcb_expect(C.c_void_p(self._h), C.c_void_p(c.ctypes.data), C.c_longlong(int(n_txps)), C.c_void_p(H.ctypes.data if H.size else None))
        if rc == -4:
            raise RuntimeError("qe_gcb_expect -4")
        _check(rc, "qe_gcb_expect")
        return H

    def window_gc(self, tids, starts, lens):
        t = np.ascontiguousarray(tids, dtype=np.uint32); s = np.ascontiguousarray(starts, dtype=np.int32); ln = np.ascontiguousarray(lens, dtype=np.int32)
        out = np.zeros(t.size, dtype=np.int32)
        _check(_lib().qe_gcb_window_gc(C.c_void_p(self._h), C.c_longlong(t.size), C.c_void_p(t.ctypes.data), C.c_void_p(s.ctypes.data), C.c_void_p(ln.ctypes.data),
                                       C.c_void_p(out.ctypes.data)), "qe_gcb_window_gc")
        return out

    def close(self):
        if self._h:
            _lib().qe_gcb_destroy(C.c_void_p(self._h)); self._h = None
