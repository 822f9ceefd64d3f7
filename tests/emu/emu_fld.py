"""tests/emu/emu_fld.py -- ctypes face of the TEST-ONLY lane emulation of the fragment-length histogram (libqm_emu_fld.so: the driver of
rapmap_amd/csrc/qm_fld_host.inl and the device code of qm_fld.inl compiled with -DQM_EMU by qm_emu_fld.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libqm_emu_fld.so")
_SRC = [os.path.join(_HERE, "qm_emu_fld.cpp")] + [os.path.join(_HERE, "../../rapmap_amd/csrc", f) for f in
                                                  ("qm_fld_host.inl", "qm_fld.inl", "qm_tally_host.inl", "qm_sweep.h", "qm_exec.h", "qm_grid.h", "qm_wave.h")] + \
       [os.path.join(_HERE, "../../include/qmap_mi355.h")]
SLAB, C_WORDS = 1024, 8
STATS = ("units", "used", "unmapped", "multi", "not_paired", "same_strand", "out_of_range", "max_len", "folds", "last_fold_us")   # the order of QM_FLD_STAT_*
PART_UNITS, PART_HITS = 1 << 22, 1 << 21                             # a part of host arrays, as qm_fld_add_hits cuts them


class ArgError(RuntimeError):
    """what the device reports as QM_E_ARG (-1)"""


def build():
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused", "-ffp-contract=off", "-o", _LIB, _SRC[0]])


def _lib():
    if not os.path.exists(_LIB) or any(os.path.getmtime(_LIB) < os.path.getmtime(s) for s in _SRC):
        build()
    lib = C.CDLL(_LIB)
    lib.qe_fld_create.restype = C.c_void_p
    for f in (lib.qe_fld_grid, lib.qe_fld_add_hits, lib.qe_fld_add_counts, lib.qe_fld_clear, lib.qe_fld_fetch, lib.qe_fld_stat):
        f.restype = C.c_int
    lib.qe_fld_destroy.restype = None
    return lib


def _check(rc, what):
    if rc == -1:
        raise ArgError("%s -1" % what)
    if rc:
        raise RuntimeError("%s failed (%d)" % (what, rc))


class EmuFld:
    """the emulated driver behind the interface of rapmap_amd.FragLenDist (what tests/fld_cases.py drives); max_units / max_hits: the
    caps of a part of add_hits' arrays (the library's by default)"""

    def __init__(self, max_len=1000, max_blocks=0, max_units=PART_UNITS, max_hits=PART_HITS):
        self.max_len, self.max_blocks, self.max_units, self.max_hits = int(max_len), int(max_blocks), int(max_units), int(max_hits)
        self._h = _lib().qe_fld_create(C.c_int(self.max_len), C.c_int(self.max_blocks))
        if not self._h:
            raise ArgError("max_len -1")

    def clear(self):
        _check(_lib().qe_fld_clear(C.c_void_p(self._h)), "qe_fld_clear")

    def add_hits(self, hit_offsets, hits):
        off = np.ascontiguousarray(hit_offsets, dtype=np.int64)
        n = len(off) - 1
        raw = None
        if hits is not None and len(hits):
            raw = np.ascontiguousarray(hits).view(np.uint8)
            assert hits.dtype.itemsize == 32 and int(off[-1]) <= len(hits)
        elif n > 0:
            assert int(off[-1]) == int(off[0])
        _check(_lib().qe_fld_add_hits(C.c_void_p(self._h), C.c_longlong(n), C.c_void_p(off.ctypes.data), C.c_void_p(raw.ctypes.data if raw is not None else None),
                                      C.c_longlong(self.max_units), C.c_longlong(self.max_hits)), "qe_fld_add_hits")

    def add_counts(self, counts):
        c = np.ascontiguousarray(counts, dtype=np.uint64)
        if c.size != self.max_len + 1:
            raise ArgError("counts -1")
        _check(_lib().qe_fld_add_counts(C.c_void_p(self._h), C.c_void_p(c.ctypes.data)), "qe_fld_add_counts")

    def counts(self):
        bins = np.zeros(SLAB, dtype=np.uint64); ctr = np.zeros(C_WORDS, dtype=np.uint64)
        _check(_lib().qe_fld_fetch(C.c_void_p(self._h), C.c_void_p(bins.ctypes.data), C.c_void_p(ctr.ctypes.data)), "qe_fld_fetch")
        assert not bins[self.max_len + 1:].any()                      # nothing lands beyond the last bin
        return bins[: self.max_len + 1].copy()

    def stat(self):
        v = C.c_int64(0); d = {}
        for which, k in enumerate(STATS):
            _check(_lib().qe_fld_stat(C.c_void_p(self._h), C.c_int(which), C.byref(v)), "qe_fld_stat")
            d[k] = int(v.value)
        return d

    def close(self):
        if self._h:
            _lib().qe_fld_destroy(C.c_void_p(self._h)); self._h = None
