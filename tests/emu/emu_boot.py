"""tests/emu/emu_boot.py -- ctypes face of the TEST-ONLY lane emulation of the bootstrap device code (libqm_emu_boot.so:
rapmap_amd/csrc/qm_boot.inl compiled with -DQM_EMU by qm_emu_boot.cpp).  Boot has the methods of rapmap_amd.Bootstrap plus
classes() (Quant.classes() on the device), so boot_cases.py drives either."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libqm_emu_boot.so")
_SRC = [os.path.join(_HERE, "qm_emu_boot.cpp")] + [os.path.join(_HERE, "../../rapmap_amd/csrc", f) for f in ("qm_boot.inl", "qm_quant.inl", "qm_eqc.inl", "qm_wave.h")]


class ArgError(RuntimeError):
    """what the device reports as QM_E_ARG"""


class StateError(RuntimeError):
    """what the device reports as QM_E_STATE"""


def build():
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused", "-ffp-contract=off", "-o", _LIB, _SRC[0]])


_lib_h = None


def _lib():
    global _lib_h
    if _lib_h is None:
        if not os.path.exists(_LIB) or any(os.path.getmtime(_LIB) < os.path.getmtime(s) for s in _SRC):
            build()
        lib = C.CDLL(_LIB)
        lib.qe_boot_create.restype = C.c_void_p
        lib.qe_boot_destroy.restype = None
        for f in (lib.qe_boot_info, lib.qe_boot_classes, lib.qe_boot_resample, lib.qe_boot_fetch, lib.qe_boot_philox):
            f.restype = None
        _lib_h = lib
    return _lib_h


def philox(counter, key):
    ctr = np.asarray(counter, dtype=np.uint32); k = np.asarray(key, dtype=np.uint32); out = np.zeros(4, dtype=np.uint32)
    _lib().qe_boot_philox(C.c_void_p(ctr.ctypes.data), C.c_void_p(k.ctypes.data), C.c_void_p(out.ctypes.data))
    return out


def _p(a):
    return C.c_void_p(a.ctypes.data if a.size else None)


class Boot:
    def __init__(self, off, tids, cnt, n_txps, eff, n_reps, aggregate=0):
        off = np.ascontiguousarray(off, dtype=np.int64); tids = np.ascontiguousarray(tids, dtype=np.uint32); cnt = np.ascontiguousarray(cnt, dtype=np.uint64)
        self.n_txps = int(n_txps); self.n_reps = int(n_reps); self._h = None
        if self.n_reps < 1:
            raise ArgError("n_reps")
        eff = np.ones(self.n_txps) if eff is None else np.ascontiguousarray(eff, dtype=np.float64)
        err = C.c_int()
        h = _lib().qe_boot_create(C.c_longlong(len(off) - 1), _p(off), _p(tids), _p(cnt), C.c_longlong(self.n_txps), _p(eff), C.c_int(self.n_reps), C.c_int(aggregate), C.byref(err))
        if err.value == -1:
            raise ArgError("a label names a transcript beyond n_txps")
        if not h:
            raise RuntimeError("qe_boot_create failed (%d)" % err.value)
        self._h = C.c_void_p(h)
        st = np.zeros(6, dtype=np.int64)
        _lib().qe_boot_info(self._h, _p(st))
        self.info = dict(zip(("classes", "entries", "present", "draws", "queued_labels", "queued_txps"), (int(x) for x in st)))
        self.launches = 0

    def classes(self):
        nc, ne = self.info["classes"], self.info["entries"]
        off = np.zeros(nc + 1, dtype=np.int64); tids = np.zeros(ne + 1, dtype=np.uint32); cnt = np.zeros(nc + 1, dtype=np.uint64)
        _lib().qe_boot_classes(self._h, _p(off), _p(tids), _p(cnt))
        return off, tids[:ne], cnt[:nc]

    def resample(self, seed=0, first_rep=0):
        _lib().qe_boot_resample(self._h, C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_longlong(int(first_rep)))

    def set_counts(self, rep, counts):
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        if counts.size != self.info["classes"]:
            raise ValueError("one count per class")
        col = np.concatenate([counts, np.zeros(1, dtype=np.uint64)])
        if _lib().qe_boot_column(self._h, C.c_int(int(rep)), _p(col), C.c_int(1)):
            raise ArgError("rep")

    def counts(self, rep):
        col = np.zeros(self.info["classes"] + 1, dtype=np.uint64)
        if _lib().qe_boot_column(self._h, C.c_int(int(rep)), _p(col), C.c_int(0)):
            raise ArgError("rep")
        return col[:-1]

    def run(self, max_iter=10000, check_every=10, rel_tol=1e-2, min_alpha=1e-8):
        it = np.zeros(self.n_reps, dtype=np.int32); rel = np.zeros(self.n_reps, dtype=np.float64); n = C.c_longlong()
        rc = _lib().qe_boot_run(self._h, C.c_int(max_iter), C.c_int(check_every), C.c_double(rel_tol), C.c_double(min_alpha), _p(it), _p(rel), C.byref(n))
        if rc == -7:
            raise StateError("no counts yet")
        self.launches = n.value
        return it, rel

    def fetch(self):
        out = np.zeros((self.n_reps, self.n_txps), dtype=np.float64)
        if out.size:
            _lib().qe_boot_fetch(self._h, _p(out))
        return out

    def close(self):
        if self._h:
            _lib().qe_boot_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()
