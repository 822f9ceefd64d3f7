"""tests/emu/emu_h2m.py -- ctypes face of the TEST-ONLY lane emulation of the lean kernel's hits-to-mappings pass
(libqm_emu_h2m.so: lean_h2m, lean_h2m_loop and lean_h2m_tiles of rapmap_amd/csrc/qm_lean.inl compiled with -DQM_EMU by qm_emu_h2m.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libqm_emu_h2m.so")
_SRC = [os.path.join(_HERE, "qm_emu_h2m.cpp"),
        os.path.join(_HERE, "../../rapmap_amd/csrc/qm_lean.inl"),
        os.path.join(_HERE, "../../rapmap_amd/csrc/qm_mapper.inl"),
        os.path.join(_HERE, "../../rapmap_amd/csrc/qm_wave.h"),
        os.path.join(_HERE, "../../include/qmap_mi355.h")]
DISPATCH, LOOP, TILES, ONE_TILE = 0, 1, 2, 3                      # `which` of qe_h2m


def build():
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unused", "-o", _LIB, _SRC[0]])


_cached = None


def _lib():
    global _cached
    if _cached is None:
        if not os.path.exists(_LIB) or any(os.path.getmtime(_LIB) < os.path.getmtime(s) for s in _SRC):
            build()
        lib = C.CDLL(_LIB)
        lib.qe_h2m.restype = C.c_int
        lib.qe_h2m_tile_lo.restype = C.c_int
        lib.qe_h2m_tile_hi.restype = C.c_int
        _cached = lib
    return _cached


def tile_range():
    """[lo, hi]: the n for which lean_h2m takes the tiles"""
    return _lib().qe_h2m_tile_lo(), _lib().qe_h2m_tile_hi()


def h2m(which, stash, m, min_idx, is_rc=False):
    """stash: (n, 4) uint32 rows {tid, pos, qp, iv} -> (count, elem[64] uint64, keep[64] bool, slot[64] int32)"""
    st = np.ascontiguousarray(stash, dtype=np.uint32).reshape(-1, 4)
    n = st.shape[0]
    elem = np.zeros(64, dtype=np.uint64); keep = np.zeros(64, dtype=np.uint8); slot = np.zeros(64, dtype=np.int32)
    cnt = _lib().qe_h2m(C.c_int(which), C.c_int(n), C.c_int(m), C.c_int(min_idx), C.c_int(1 if is_rc else 0), C.c_void_p(st.ctypes.data),
                        C.c_void_p(elem.ctypes.data), C.c_void_p(keep.ctypes.data), C.c_void_p(slot.ctypes.data))
    if cnt < 0:
        raise ValueError("qe_h2m: bad argument (which %d, n %d, m %d, minIdx %d)" % (which, n, m, min_idx))
    return cnt, elem, keep.astype(bool), slot
