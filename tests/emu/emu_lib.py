"""tests/emu/emu_lib.py -- ctypes face of the TEST-ONLY lane emulation of the library-type sweep (libqm_emu_lib.so: the driver of
rapmap_amd/csrc/qm_lib_host.inl and the device code of qm_lib.inl compiled with -DQM_EMU by qm_emu_lib.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

from lib_cases import mask_of

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libqm_emu_lib.so")
_SRC = [os.path.join(_HERE, "qm_emu_lib.cpp")] + [os.path.join(_HERE, "../../rapmap_amd/csrc", f) for f in
                                                  ("qm_lib_host.inl", "qm_lib.inl", "qm_eqc_host.inl", "qm_eqc.inl", "qm_tally_host.inl", "qm_sweep.h", "qm_exec.h", "qm_grid.h", "qm_wave.h")] + \
       [os.path.join(_HERE, "../../include/qmap_mi355.h")]


class ArgError(RuntimeError):
    """what the device reports as QM_E_ARG (-1)"""


def build():
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused", "-o", _LIB, _SRC[0]])


def _lib():
    if not os.path.exists(_LIB) or any(os.path.getmtime(_LIB) < os.path.getmtime(s) for s in _SRC):
        build()
    lib = C.CDLL(_LIB)
    lib.qe_lib_add.restype = C.c_int
    lib.qe_lib_grid.restype = C.c_int
    lib.qe_lib_eqc.restype = C.c_longlong
    return lib


PART_UNITS, PART_HITS = 1 << 22, 1 << 21                             # a part of host arrays, as qm_lib_add_hits cuts them


def _arrays(hit_offsets, hits):
    """offsets rebased to 0 and the bytes of the hits they cover, as a sweep is handed them on the device"""
    off = np.ascontiguousarray(hit_offsets, dtype=np.int64)
    n = len(off) - 1
    raw = None
    if hits is not None and len(hits):
        assert hits.dtype.itemsize == 32 and int(off[-1]) <= len(hits)
        raw = np.ascontiguousarray(hits[int(off[0]):int(off[-1])]).view(np.uint8) if n > 0 and off[-1] > off[0] else None
    elif n > 0:
        assert int(off[-1]) == int(off[0])
    return off - off[0] if n >= 0 else off, n, raw


class EmuLib:
    """the emulated driver behind the interface of rapmap_amd.LibFormat (what tests/lib_cases.py drives); max_units / max_hits: the
    caps of a part of the host arrays (the library's by default)"""

    def __init__(self, lib_type="A", max_blocks=0, max_units=PART_UNITS, max_hits=PART_HITS):
        self.mask = mask_of(lib_type)
        if not 0 < self.mask <= 0xfff:
            raise ArgError("mask -1")
        self.max_blocks, self.max_units, self.max_hits = int(max_blocks), int(max_units), int(max_hits)
        self.clear()

    def clear(self):
        self._ctr = np.zeros(32, dtype=np.uint64); self._sweeps = 0

    def _sweep(self, hit_offsets, hits, lists):
        # the arrays as the caller has them: the driver rebases the offsets part by part
        off = np.ascontiguousarray(hit_offsets, dtype=np.int64)
        n = len(off) - 1
        raw = None
        if hits is not None and len(hits):
            assert hits.dtype.itemsize == 32 and int(off[-1]) <= len(hits)
            raw = np.ascontiguousarray(hits).view(np.uint8)
        elif n > 0:
            assert int(off[-1]) == int(off[0])
        new_off = np.zeros(max(n, 0) + 1, dtype=np.int64); tids = np.zeros(max(int(off[-1] - off[0]), 0) + 1 if n > 0 else 1, dtype=np.uint32)
        sweeps = C.c_longlong(0)
        rc = _lib().qe_lib_add(C.c_longlong(n), C.c_void_p(off.ctypes.data), C.c_void_p(raw.ctypes.data if raw is not None else None),
                               C.c_uint32(self.mask), C.c_int(self.max_blocks), C.c_longlong(self.max_units), C.c_longlong(self.max_hits),
                               C.c_void_p(self._ctr.ctypes.data), C.c_void_p(new_off.ctypes.data if lists else None),
                               C.c_void_p(tids.ctypes.data if lists else None), C.byref(sweeps))
        self._sweeps += sweeps.value
        if rc == -1:
            raise ArgError("qe_lib_add -1")
        if rc:
            raise RuntimeError("qe_lib_add failed (%d)" % rc)
        return new_off, tids[:int(new_off[-1])].copy()

    def add_hits(self, hit_offsets, hits):
        self._sweep(hit_offsets, hits, False)

    def compact_hits(self, hit_offsets, hits):
        return self._sweep(hit_offsets, hits, True)

    def add_counts(self, counts):
        c = np.ascontiguousarray(counts, dtype=np.uint64)
        if c.size != 32 or c[31]:
            raise ArgError("counts -1")
        self._ctr += c

    def counts(self):
        return self._ctr.copy()

    def stat(self):
        return {"sweeps": self._sweeps, "last_sweep_us": 0, "mask": self.mask}

    def close(self):
        pass


def eqc_add_lib(hit_offsets, hits, lib_type, max_blocks=0):
    """qm_eqc_add_lib's fold into a fresh table -> ((label_offsets, tids, counts), tallies uint64[32])"""
    off, n, raw = _arrays(hit_offsets, hits)
    ctr = np.zeros(32, dtype=np.uint64)
    out_off = np.zeros(n + 2, dtype=np.int64); out_tids = np.zeros(int(off[-1]) + 1, dtype=np.uint32); out_cnt = np.zeros(n + 1, dtype=np.uint64)
    nc = _lib().qe_lib_eqc(C.c_longlong(n), C.c_void_p(off.ctypes.data), C.c_void_p(raw.ctypes.data if raw is not None else None), C.c_int(32),
                           C.c_uint32(mask_of(lib_type)), C.c_int(max_blocks), C.c_void_p(ctr.ctypes.data), C.c_void_p(out_off.ctypes.data),
                           C.c_void_p(out_tids.ctypes.data), C.c_void_p(out_cnt.ctypes.data))
    if nc < 0:
        raise RuntimeError("qe_lib_eqc failed (%d)" % nc)
    return (out_off[: nc + 1].copy(), out_tids[: int(out_off[nc])].copy(), out_cnt[:nc].copy()), ctr
