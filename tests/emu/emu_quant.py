"""tests/emu/emu_quant.py -- ctypes face of the TEST-ONLY lane emulation of the abundance-estimation device code (libqm_emu_quant.so:
rapmap_amd/csrc/qm_quant.inl compiled with -DQM_EMU by qm_emu_quant.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libqm_emu_quant.so")
_SRC = [os.path.join(_HERE, "qm_emu_quant.cpp"),
        os.path.join(_HERE, "../../rapmap_amd/csrc/qm_quant.inl"),
        os.path.join(_HERE, "../../rapmap_amd/csrc/qm_eqc.inl"),
        os.path.join(_HERE, "../../rapmap_amd/csrc/qm_wave.h")]
STATS = ("classes", "entries", "present", "longest_label", "longest_list", "queued_labels", "queued_txps", "iterations")


class ArgError(RuntimeError):
    """what the device reports as QM_E_ARG"""


def build():
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused", "-ffp-contract=off", "-o", _LIB, _SRC[0]])


def _lib():
    if not os.path.exists(_LIB) or any(os.path.getmtime(_LIB) < os.path.getmtime(s) for s in _SRC):
        build()
    lib = C.CDLL(_LIB)
    lib.qe_quant_run.restype = C.c_int
    return lib


def run(off, tids, cnt, n_txps, eff=None, alpha0=None, max_iter=10000, check_every=10, rel_tol=1e-2, min_alpha=1e-8):
    """the structure build and the EM over a table given as canonical arrays -> (alpha, iterations, last_rel_change, stats)"""
    off = np.ascontiguousarray(off, dtype=np.int64); tids = np.ascontiguousarray(tids, dtype=np.uint32); cnt = np.ascontiguousarray(cnt, dtype=np.uint64)
    n_txps = int(n_txps)
    eff = np.ones(n_txps) if eff is None else np.ascontiguousarray(eff, dtype=np.float64)
    if eff.size != n_txps or not (np.isfinite(eff).all() and (eff > 0).all()):
        raise ArgError("effective lengths")
    if alpha0 is not None:
        alpha0 = np.ascontiguousarray(alpha0, dtype=np.float64)
        if alpha0.size != n_txps or not (np.isfinite(alpha0).all() and (alpha0 >= 0).all()):
            raise ArgError("start values")
    out = np.zeros(n_txps + 1, dtype=np.float64); rel = C.c_double(); stats = np.zeros(8, dtype=np.int64)
    rc = _lib().qe_quant_run(C.c_longlong(len(off) - 1), C.c_void_p(off.ctypes.data), C.c_void_p(tids.ctypes.data if tids.size else None),
                             C.c_void_p(cnt.ctypes.data if cnt.size else None), C.c_longlong(n_txps), C.c_void_p(eff.ctypes.data if n_txps else None),
                             C.c_void_p(alpha0.ctypes.data if alpha0 is not None and n_txps else None), C.c_int(max_iter), C.c_int(check_every),
                             C.c_double(rel_tol), C.c_double(min_alpha), C.c_void_p(out.ctypes.data), C.byref(rel), C.c_void_p(stats.ctypes.data))
    if rc == -1:
        raise ArgError("a label names a transcript beyond n_txps")
    if rc:
        raise RuntimeError("qe_quant_run failed (%d)" % rc)
    st = dict(zip(STATS, (int(x) for x in stats)))
    return out[:n_txps].copy(), st["iterations"], rel.value, st
