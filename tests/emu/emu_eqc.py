"""tests/emu/emu_eqc.py -- ctypes face of the TEST-ONLY lane emulation of the equivalence-class device code (libqm_emu_eqc.so:
rapmap_amd/csrc/qm_eqc.inl compiled with -DQM_EMU by qm_emu_eqc.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libqm_emu_eqc.so")
_SRC = [os.path.join(_HERE, "qm_emu_eqc.cpp")] + [os.path.join(_HERE, "../../rapmap_amd/csrc", f) for f in ("qm_eqc_host.inl", "qm_exec.h", "qm_eqc.inl", "qm_wave.h")]


class ArgError(RuntimeError):
    """what the device reports as QM_E_ARG (-1)"""


def build():
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused", "-o", _LIB, _SRC[0]])


def _lib():
    if not os.path.exists(_LIB) or any(os.path.getmtime(_LIB) < os.path.getmtime(s) for s in _SRC):
        build()
    lib = C.CDLL(_LIB)
    lib.qe_eqc_run.restype = C.c_longlong
    return lib


def run(offsets, tids, weights=None, hash_bits=0, cap=16, pool_cap=64, long_cap=4, aggregate=True, folds=1, stride=4, max_units=0, max_tids=0):
    """the label and insert stages over n lists -> (label_offsets, tids, counts, stats); stride=32: the tids sit in the first
    word of 32-byte records, as in an array of hits.  max_units > 0: through qm_eqc_add_labels' driver, the host arrays in parts of at
    most max_units lists and max_tids tids (offsets[0] need not be 0).  stats: growths, collision_probes, long_units, rounds"""
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    no_tids = tids is None                                        # a null pointer: lists without a tid need no array
    tids = np.ascontiguousarray([] if no_tids else tids, dtype=np.uint32)
    n = len(offsets) - 1
    src = tids
    if stride != 4:
        src = np.zeros((tids.size + 1) * (stride // 4), dtype=np.uint32)
        src[: tids.size * (stride // 4): stride // 4] = tids
        src[1::stride // 4] = 0xdeadbeef                          # what follows a tid in its record must not matter
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint64)
    out_off = np.zeros(n + 2, dtype=np.int64); out_tids = np.zeros(tids.size + 1, dtype=np.uint32); out_cnt = np.zeros(n + 1, dtype=np.uint64)
    stats = np.zeros(4, dtype=np.int64)
    nc = _lib().qe_eqc_run(C.c_longlong(n), C.c_void_p(offsets.ctypes.data), C.c_void_p(None if no_tids else src.ctypes.data), C.c_int(stride),
                           C.c_void_p(w.ctypes.data if w is not None else None), C.c_int(hash_bits), C.c_uint64(cap), C.c_uint64(pool_cap),
                           C.c_longlong(long_cap), C.c_int(1 if aggregate else 0), C.c_int(folds), C.c_longlong(max_units), C.c_longlong(max_tids), C.c_void_p(out_off.ctypes.data),
                           C.c_void_p(out_tids.ctypes.data), C.c_void_p(out_cnt.ctypes.data), C.c_void_p(stats.ctypes.data))
    if nc == -1:
        raise ArgError("qe_eqc_run -1")
    if nc < 0:
        raise RuntimeError("qe_eqc_run failed (%d)" % nc)
    nt = int(out_off[nc])
    return out_off[: nc + 1].copy(), out_tids[:nt].copy(), out_cnt[:nc].copy(), dict(zip(("growths", "collision_probes", "long_units", "rounds"), (int(x) for x in stats)))
