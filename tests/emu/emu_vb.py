"""tests/emu/emu_vb.py -- ctypes face of the TEST-ONLY lane emulation of the variational Bayes method (libqm_emu_vb.so: the drivers and
the device code of the quant and the boot object compiled with -DQM_EMU by qm_emu_vb.cpp).  Quant and Boot have the methods of
rapmap_amd.Quant and rapmap_amd.Bootstrap that vb_cases.py uses, so it drives either."""
import ctypes as C
import os
import subprocess

import numpy as np

import emu_boot
import emu_quant

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libqm_emu_vb.so")
_SRC = [os.path.join(_HERE, "qm_emu_vb.cpp")] + emu_boot._SRC
ArgError, StateError, check = emu_quant.ArgError, emu_quant.StateError, emu_quant.check
METHODS = {"em": 0, "vbem": 1}


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
        for f in (lib.qe_boot_destroy, lib.qe_boot_info):
            f.restype = None
        _lib_h = lib
    return _lib_h


def _p(a):
    return C.c_void_p(a.ctypes.data if a is not None and a.size else None)


def exp_digamma(x):
    x = np.ascontiguousarray(x, dtype=np.float64); out = np.zeros(x.shape, dtype=np.float64)
    check(_lib().qe_exp_digamma(_p(x), C.c_longlong(x.size), _p(out)), "qe_exp_digamma")
    return out


class Quant(emu_quant.Quant):
    def __init__(self, off, tids, cnt, n_txps, eff=None):
        super().__init__(off, tids, cnt, n_txps, eff, lib=_lib())

    def set_method_code(self, code, prior=None):
        if prior is not None:
            prior = np.ascontiguousarray(prior, dtype=np.float64)
            if prior.size != self.n_txps:
                raise ValueError("one prior per transcript")
        check(self._l.qe_quant_set_method(self._h, C.c_int(int(code)), _p(prior)), "qe_quant_set_method")

    def set_method(self, method="em", prior=None):
        self.set_method_code(METHODS[method], prior)

    def classes(self):
        st = self.stat()
        off = np.zeros(st["classes"] + 1, dtype=np.int64); tids = np.zeros(st["entries"], dtype=np.uint32); cnt = np.zeros(st["classes"], dtype=np.uint64)
        check(self._l.qe_quant_classes(self._h, _p(off), _p(tids), _p(cnt)), "qe_quant_classes")
        return off, tids, cnt


class Boot:
    """the methods of rapmap_amd.Bootstrap over a Quant of this module"""

    def __init__(self, quant, n_reps):
        self.quant, self.n_txps, self.n_reps, self._h = quant, quant.n_txps, int(n_reps), None
        err = C.c_int()
        h = _lib().qe_boot_create(quant._h, C.c_int(self.n_reps), C.c_int(0), C.byref(err))
        check(err.value, "qe_boot_create")
        self._h = C.c_void_p(h)
        self.n_classes = quant.stat()["classes"]

    def resample(self, seed=0, first_rep=0):
        check(_lib().qe_boot_resample(self._h, C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_longlong(int(first_rep))), "qe_boot_resample")

    def set_counts(self, rep, counts):
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        if counts.size != self.n_classes:
            raise ValueError("one count per class")
        check(_lib().qe_boot_set_counts(self._h, C.c_int(int(rep)), _p(counts)), "qe_boot_set_counts")

    def counts(self, rep):
        col = np.zeros(self.n_classes, dtype=np.uint64)
        check(_lib().qe_boot_fetch_counts(self._h, C.c_int(int(rep)), _p(col)), "qe_boot_fetch_counts")
        return col

    def run(self, max_iter=10000, check_every=10, rel_tol=1e-2, min_alpha=1e-8):
        it = np.zeros(self.n_reps, dtype=np.int32); rel = np.zeros(self.n_reps, dtype=np.float64); n = C.c_longlong()
        check(_lib().qe_boot_run(self._h, C.c_int(max_iter), C.c_int(check_every), C.c_double(rel_tol), C.c_double(min_alpha), _p(it), _p(rel), C.byref(n)), "qe_boot_run")
        return it, rel

    def fetch(self):
        out = np.zeros((self.n_reps, self.n_txps), dtype=np.float64)
        check(_lib().qe_boot_fetch(self._h, _p(out)), "qe_boot_fetch")
        return out

    def close(self):
        if self._h:
            _lib().qe_boot_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()
