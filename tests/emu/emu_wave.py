"""tests/emu/emu_wave.py -- ctypes face of the TEST-ONLY lane emulation of the primitives (libqm_emu_wave.so: tests/device/qm_wave_probe.inl,
one call of every primitive of rapmap_amd/csrc/qm_wave.h and of key_count, compiled with -DQM_EMU by qm_emu_wave.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libqm_emu_wave.so")
_SRC = [os.path.join(_HERE, "qm_emu_wave.cpp"),
        os.path.join(_HERE, "../device/qm_wave_probe.inl"),
        os.path.join(_HERE, "../../rapmap_amd/csrc/qm_wave.h"),
        os.path.join(_HERE, "../../rapmap_amd/csrc/qm_mapper.inl"),
        os.path.join(_HERE, "../../rapmap_amd/csrc/qm_sel.inl"),
        os.path.join(_HERE, "../../rapmap_amd/csrc/qm_selpack.inl"),
        os.path.join(_HERE, "../../rapmap_amd/csrc/qm_sweep.h"),
        os.path.join(_HERE, "../../rapmap_amd/csrc/qm_lib.inl"),
        os.path.join(_HERE, "../../include/qmap_mi355.h")]


def build():
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused", "-o", _LIB, _SRC[0]])


_cached = None


def _lib():
    global _cached
    if _cached is None:
        if not os.path.exists(_LIB) or any(os.path.getmtime(_LIB) < os.path.getmtime(s) for s in _SRC):
            build()
        lib = C.CDLL(_LIB)
        lib.qe_wave.restype = C.c_int
        lib.qe_op_name.restype = C.c_char_p
        _cached = lib
    return _cached


def ops():
    """{name: number} of the probe body's ops"""
    lib = _lib()
    return {lib.qe_op_name(i).decode(): i for i in range(lib.qe_n_ops())}


def sizes():
    """(bytes of memory per wave, output rows)"""
    return _lib().qe_memb(), _lib().qe_nout()


def call_wave(fn, ops_, memb, nout, op, prm, a, b, c, d, mem, atom):
    """the one argument layout of qe_wave and the device probe's qp_wave -> (out[W, nout, 64] uint64, atom[W] uint64, return code)"""
    prm = np.ascontiguousarray(prm, dtype=np.int32)
    nw = len(prm)
    arr = [np.ascontiguousarray(x, dtype=np.uint64) for x in (a, b, c, d)]
    mem = np.ascontiguousarray(mem, dtype=np.uint8)
    assert all(x.shape == (nw, 64) for x in arr) and mem.shape == (nw, memb)
    atom = np.array(atom, dtype=np.uint64)                                    # (a copy: the call writes it)
    assert atom.shape == (nw,)
    out = np.zeros((nw, nout, 64), dtype=np.uint64)
    rc = fn(C.c_int(ops_[op]), C.c_int(nw), C.c_void_p(prm.ctypes.data), *[C.c_void_p(x.ctypes.data) for x in arr], C.c_void_p(mem.ctypes.data),
            C.c_void_p(atom.ctypes.data), C.c_void_p(out.ctypes.data))
    return out, atom, rc


def wave(op, prm, a, b, c, d, mem, atom):
    memb, nout = sizes()
    out, atom, rc = call_wave(_lib().qe_wave, ops(), memb, nout, op, prm, a, b, c, d, mem, atom)
    if rc:
        raise ValueError("qe_wave: bad argument (op %s)" % op)
    return out, atom
