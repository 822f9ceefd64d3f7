"""tests/emu/emu_boot.py -- ctypes face of the TEST-ONLY lane emulation of the bootstrap device code (libqm_emu_boot.so:
rapmap_amd/csrc/qm_boot.inl compiled with -DQM_EMU by qm_emu_boot.cpp).  Boot has the methods of rapmap_amd.Bootstrap plus
classes() (Quant.classes() on the device), so boot_cases.py drives either."""
import ctypes as C
import os
import subprocess

import numpy as np

import emu_quant

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libqm_emu_boot.so")
_SRC = [os.path.join(_HERE, "qm_emu_boot.cpp"), os.path.join(_HERE, "qm_emu_quant.cpp")] + [os.path.join(_HERE, "../../rapmap_amd/csrc", f) for f in (
    "qm_boot_host.inl", "qm_quant_host.inl", "qm_eqc_host.inl", "qm_exec.h", "qm_boot.inl", "qm_quant.inl", "qm_eqc.inl", "qm_wave.h")]
ArgError, StateError, check = emu_quant.ArgError, emu_quant.StateError, emu_quant.check


def build():
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused", "-ffp-contract=off", "-o", _LIB, _SRC[0]])


_lib_h = None


def _lib():
    global _lib_h
    if _lib_h is None:
        if not os.path.exists(_LIB) or any(os.path.getmtime(_LIB) < os.path.getmtime(s) for s in _SRC):
            build()
        lib = emu_quant.declare(C.CDLL(_LIB))
        lib.qe_boot_create.restype = C.c_void_p
        for f in (lib.qe_boot_destroy, lib.qe_boot_info, lib.qe_boot_philox):
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
    """over a quant object of its own, made from the canonical arrays, or over `quant` (an emu_quant.Quant made with lib=emu_boot._lib())"""

    def __init__(self, off, tids, cnt, n_txps, eff, n_reps, aggregate=0, quant=None):
        self.n_txps = int(n_txps); self.n_reps = int(n_reps); self._h = None
        self.quant = quant or emu_quant.Quant(off, tids, cnt, n_txps, eff, lib=_lib()); self._own = quant is None
        err = C.c_int()
        h = _lib().qe_boot_create(self.quant._h, C.c_int(self.n_reps), C.c_int(aggregate), C.byref(err))
        if err.value and self._own:
            self.quant.close()
        check(err.value, "qe_boot_create")
        self._h = C.c_void_p(h)
        st = np.zeros(6, dtype=np.int64)
        _lib().qe_boot_info(self._h, _p(st))
        self.info = dict(zip(("classes", "entries", "present", "draws", "queued_labels", "queued_txps"), (int(x) for x in st)))
        self.launches = 0

    def classes(self):
        nc, ne = self.info["classes"], self.info["entries"]
        off = np.zeros(nc + 1, dtype=np.int64); tids = np.zeros(ne, dtype=np.uint32); cnt = np.zeros(nc, dtype=np.uint64)
        check(_lib().qe_boot_classes(self._h, _p(off), _p(tids), _p(cnt)), "qe_boot_classes")
        return off, tids, cnt

    def resample(self, seed=0, first_rep=0):
        check(_lib().qe_boot_resample(self._h, C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_longlong(int(first_rep))), "qe_boot_resample")

    def set_counts(self, rep, counts):
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        if counts.size != self.info["classes"]:
            raise ValueError("one count per class")
        check(_lib().qe_boot_set_counts(self._h, C.c_int(int(rep)), _p(counts)), "qe_boot_set_counts")

    def counts(self, rep):
        col = np.zeros(self.info["classes"], dtype=np.uint64)
        check(_lib().qe_boot_fetch_counts(self._h, C.c_int(int(rep)), _p(col)), "qe_boot_fetch_counts")
        return col

    def run(self, max_iter=10000, check_every=10, rel_tol=1e-2, min_alpha=1e-8):
        it = np.zeros(self.n_reps, dtype=np.int32); rel = np.zeros(self.n_reps, dtype=np.float64); n = C.c_longlong()
        check(_lib().qe_boot_run(self._h, C.c_int(max_iter), C.c_int(check_every), C.c_double(rel_tol), C.c_double(min_alpha), _p(it), _p(rel), C.byref(n)), "qe_boot_run")
        self.launches = n.value
        return it, rel

    def fetch(self):
        out = np.zeros((self.n_reps, self.n_txps), dtype=np.float64)
        check(_lib().qe_boot_fetch(self._h, _p(out)), "qe_boot_fetch")
        return out

    def close(self):
        if self._h:
            _lib().qe_boot_destroy(self._h)
            self._h = None
            if self._own:
                self.quant.close()

    def __del__(self):
        self.close()
