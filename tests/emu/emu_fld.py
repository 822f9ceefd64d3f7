"""tests/emu/emu_fld.py -- ctypes face of the TEST-ONLY lane emulation of the fragment-length sweep (libqm_emu_fld.so:
rapmap_amd/csrc/qm_fld.inl compiled with -DQM_EMU by qm_emu_fld.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libqm_emu_fld.so")
_SRC = [os.path.join(_HERE, "qm_emu_fld.cpp"),
        os.path.join(_HERE, "../../rapmap_amd/csrc/qm_fld.inl"),
        os.path.join(_HERE, "../../rapmap_amd/csrc/qm_wave.h"),
        os.path.join(_HERE, "../../include/qmap_mi355.h")]
SLAB, C_WORDS = 1024, 8
CATS = ("used", "unmapped", "multi", "not_paired", "same_strand", "out_of_range")     # the order of FLD_C_*


class ArgError(RuntimeError):
    """what the device reports as QM_E_ARG (-1)"""


def build():
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused", "-ffp-contract=off", "-o", _LIB, _SRC[0]])


def _lib():
    if not os.path.exists(_LIB) or any(os.path.getmtime(_LIB) < os.path.getmtime(s) for s in _SRC):
        build()
    lib = C.CDLL(_LIB)
    lib.qe_fld_fold.restype = C.c_int
    lib.qe_fld_grid.restype = C.c_int
    return lib


class EmuFld:
    """the emulated sweep behind the interface of rapmap_amd.FragLenDist (what tests/fld_cases.py drives)"""

    def __init__(self, max_len=1000, max_blocks=0):
        if not 1 <= max_len <= SLAB - 1:
            raise ArgError("max_len -1")
        self.max_len, self.max_blocks = int(max_len), int(max_blocks)
        self.clear()

    def clear(self):
        self._bins = np.zeros(SLAB, dtype=np.uint64); self._ctr = np.zeros(C_WORDS, dtype=np.uint64)
        self._units = 0; self._folds = 0

    def add_hits(self, hit_offsets, hits):
        off = np.ascontiguousarray(hit_offsets, dtype=np.int64)
        n = len(off) - 1
        raw = None
        if hits is not None and len(hits):
            raw = np.ascontiguousarray(hits).view(np.uint8)
            assert hits.dtype.itemsize == 32 and int(off[-1]) <= len(hits)
        elif n > 0:
            assert int(off[-1]) == int(off[0])
        rc = _lib().qe_fld_fold(C.c_longlong(n), C.c_void_p(off.ctypes.data), C.c_void_p(raw.ctypes.data if raw is not None else None), C.c_int(32),
                                C.c_int(self.max_len), C.c_int(self.max_blocks), C.c_void_p(self._bins.ctypes.data), C.c_void_p(self._ctr.ctypes.data))
        if rc:
            raise RuntimeError("qe_fld_fold failed (%d)" % rc)
        if n > 0:
            self._units += n; self._folds += 1

    def add_counts(self, counts):
        c = np.ascontiguousarray(counts, dtype=np.uint64)
        if c.size != self.max_len + 1 or c[0]:
            raise ArgError("counts -1")
        self._bins[: c.size] += c
        self._ctr[0] += c.sum(); self._units += int(c.sum())

    def counts(self):
        assert not self._bins[self.max_len + 1:].any()                # nothing lands beyond the last bin
        return self._bins[: self.max_len + 1].copy()

    def stat(self):
        d = {"units": self._units}
        d.update((k, int(self._ctr[i])) for i, k in enumerate(CATS))
        d.update(max_len=self.max_len, folds=self._folds, last_fold_us=0)
        return d

    def close(self):
        pass
