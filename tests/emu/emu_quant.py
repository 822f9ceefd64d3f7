"""tests/emu/emu_quant.py -- ctypes face of the TEST-ONLY lane emulation of the abundance-estimation device code (libqm_emu_quant.so:
rapmap_amd/csrc/qm_quant.inl compiled with -DQM_EMU by qm_emu_quant.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libqm_emu_quant.so")
_SRC = [os.path.join(_HERE, "qm_emu_quant.cpp")] + [os.path.join(_HERE, "../../rapmap_amd/csrc", f) for f in (
    "qm_quant_host.inl", "qm_eqc_host.inl", "qm_exec.h", "qm_quant.inl", "qm_eqc.inl", "qm_wave.h")]
STATS = ("classes", "entries", "present", "longest_label", "longest_list", "queued_labels", "queued_txps", "iterations")
QM_E_ARG, QM_E_STATE = -1, -7


class ArgError(RuntimeError):
    """what the device reports as QM_E_ARG"""


class StateError(RuntimeError):
    """what the device reports as QM_E_STATE"""


def check(rc, what):
    if rc:
        raise {QM_E_ARG: ArgError, QM_E_STATE: StateError}.get(rc, RuntimeError)("%s failed (%d)" % (what, rc))


def build():
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused", "-ffp-contract=off", "-o", _LIB, _SRC[0]])


_lib_h = None


def _lib():
    global _lib_h
    if _lib_h is None:
        if not os.path.exists(_LIB) or any(os.path.getmtime(_LIB) < os.path.getmtime(s) for s in _SRC):
            build()
        _lib_h = declare(C.CDLL(_LIB))
    return _lib_h


def declare(lib):
    lib.qe_quant_create.restype = C.c_void_p
    lib.qe_quant_stats.restype = None
    return lib


def _p(a):
    return C.c_void_p(a.ctypes.data if a is not None and a.size else None)


class Quant:
    """the methods of rapmap_amd.Quant over a table given as canonical arrays; lib: the library that holds the object (emu_boot's own,
    for a quant object that a Boot borrows)"""

    def __init__(self, off, tids, cnt, n_txps, eff=None, lib=None):
        off = np.ascontiguousarray(off, dtype=np.int64); tids = np.ascontiguousarray(tids, dtype=np.uint32); cnt = np.ascontiguousarray(cnt, dtype=np.uint64)
        self.n_txps = int(n_txps); self._h = None; self._l = lib or _lib()
        if eff is not None:
            eff = np.ascontiguousarray(eff, dtype=np.float64)
            if eff.size != self.n_txps:
                raise ValueError("one effective length per transcript")
        err = C.c_int()
        h = self._l.qe_quant_create(C.c_longlong(len(off) - 1), _p(off), _p(tids), _p(cnt), C.c_longlong(self.n_txps), _p(eff), C.byref(err))
        check(err.value, "qe_quant_create")
        self._h = C.c_void_p(h)

    def set_start(self, alpha0=None):
        if alpha0 is not None:
            alpha0 = np.ascontiguousarray(alpha0, dtype=np.float64)
            if alpha0.size != self.n_txps:
                raise ValueError("one start value per transcript")
        check(self._l.qe_quant_set_start(self._h, _p(alpha0)), "qe_quant_set_start")

    def run(self, max_iter=10000, check_every=10, rel_tol=1e-2, min_alpha=1e-8):
        it = C.c_int(); rel = C.c_double()
        check(self._l.qe_quant_run(self._h, C.c_int(max_iter), C.c_int(check_every), C.c_double(rel_tol), C.c_double(min_alpha), C.byref(it), C.byref(rel)), "qe_quant_run")
        return it.value, rel.value

    def fetch(self):
        out = np.zeros(self.n_txps, dtype=np.float64)
        check(self._l.qe_quant_fetch(self._h, _p(out)), "qe_quant_fetch")
        return out

    def stat(self):
        st = np.zeros(7, dtype=np.int64)
        self._l.qe_quant_stats(self._h, _p(st))
        return dict(zip(STATS, (int(x) for x in st)))

    def close(self):
        """raises StateError, and destroys nothing, while a Boot borrows the object"""
        if self._h:
            check(self._l.qe_quant_destroy(self._h), "qe_quant_destroy")
            self._h = None

    def __del__(self):
        try:
            self.close()
        except StateError:
            pass


def run(off, tids, cnt, n_txps, eff=None, alpha0=None, max_iter=10000, check_every=10, rel_tol=1e-2, min_alpha=1e-8):
    """the structure build and the EM over a table given as canonical arrays -> (alpha, iterations, last_rel_change, stats)"""
    q = Quant(off, tids, cnt, n_txps, eff)
    try:
        if alpha0 is not None:
            q.set_start(alpha0)
        it, rel = q.run(max_iter, check_every, rel_tol, min_alpha)
        st = q.stat(); st["iterations"] = it
        return q.fetch(), it, rel, st
    finally:
        q.close()
