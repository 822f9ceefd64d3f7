"""tests/emu/emu_sel.py -- ctypes face of the TEST-ONLY lane emulation of the -s question scorer and the strip alignments by themselves
(libqm_emu_sel.so: sel_side_score<1> with SelRedOne and sel_tasks_strip of rapmap_amd/csrc/qm_sel.inl compiled with -DQM_EMU by qm_emu_sel.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libqm_emu_sel.so")
_SRC = [os.path.join(_HERE, "qm_emu_sel.cpp"),
        os.path.join(_HERE, "../../rapmap_amd/csrc/qm_sel.inl"),
        os.path.join(_HERE, "../../rapmap_amd/csrc/qm_selpack.inl"),
        os.path.join(_HERE, "../../rapmap_amd/csrc/qm_mapper.inl"),
        os.path.join(_HERE, "../../rapmap_amd/csrc/qm_wave.h"),
        os.path.join(_HERE, "../../include/qmap_mi355.h")]
NEVER = 0x5A5A5A5A                                                # tsc of a question nobody wrote
TASK_FIELDS = ("written", "rd", "tx", "gslot", "rl", "roff", "rlen", "tlen1", "fwd")


def build():
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused", "-o", _LIB, _SRC[0]])


_cached = None


def _lib():
    global _cached
    if _cached is None:
        if not os.path.exists(_LIB) or any(os.path.getmtime(_LIB) < os.path.getmtime(s) for s in _SRC):
            build()
        lib = C.CDLL(_LIB)
        lib.qe_sel_side.restype = C.c_int
        _cached = lib
    return _cached


def max_read_len():
    return _lib().qe_sel_max_read_len()


def flat(batch):
    """the arrays both faces hand over (tests/sel_side_cases.py: Batch) -> (reads, roffs, text, txp_off, txp_len, qd)"""
    return (np.ascontiguousarray(batch.reads, dtype=np.uint8), np.ascontiguousarray(batch.roffs, dtype=np.int64),
            np.ascontiguousarray(batch.text, dtype=np.uint8), np.ascontiguousarray(batch.txp_off, dtype=np.uint32),
            np.ascontiguousarray(batch.txp_len, dtype=np.int32), np.ascontiguousarray(batch.qd, dtype=np.int32).reshape(-1, 5))


def sel_side(batch, policy, scheme, strip=True):
    """every question of the batch through sel_side_score<1>, then (strip) the questions with kind & 4 through sel_tasks_strip four at a time
    -> (kind[n] int32, tsc[n] int32, key[n] uint64, task[n, 9] int64 rows of TASK_FIELDS, number of strip alignments)"""
    reads, roffs, text, txp_off, txp_len, qd = flat(batch)
    n = len(qd)
    a, b, q_, e_, w = scheme
    prm = np.array([policy, a, b, q_, e_, w, 1 if strip else 0], dtype=np.int32)
    kind = np.zeros(n, dtype=np.int32); tsc = np.zeros(n, dtype=np.int32); key = np.zeros(n, dtype=np.uint64); task = np.zeros((n, 9), dtype=np.int64)
    rc = _lib().qe_sel_side(C.c_int(n), C.c_void_p(reads.ctypes.data), C.c_void_p(roffs.ctypes.data), C.c_void_p(text.ctypes.data),
                            C.c_longlong(len(text)), C.c_int(len(txp_off)), C.c_void_p(txp_off.ctypes.data), C.c_void_p(txp_len.ctypes.data),
                            C.c_void_p(qd.ctypes.data), C.c_void_p(prm.ctypes.data), C.c_void_p(kind.ctypes.data), C.c_void_p(tsc.ctypes.data),
                            C.c_void_p(key.ctypes.data), C.c_void_p(task.ctypes.data))
    if rc < 0:
        raise ValueError("qe_sel_side: bad argument")
    return kind, tsc, key, task, rc
