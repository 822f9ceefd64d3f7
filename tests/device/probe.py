"""tests/device/probe.py -- ctypes face of the TEST-ONLY device probes (libqm_probe.so, tests/device/qm_probe.hip): single wave bodies of the
product's source run by themselves on the GPU -- the primitives of qm_wave.h, lean_h2m, the ksw2 row kernels, the -s question scorer and the
strip alignments -- so that the device edition of
each can be held to its lane emulation (tests/emu).  The library is rebuilt when a source is newer; a missing library that cannot be built is
an error, not a skip.  Load it after torch has opened the device (the `lib_built` fixture of tests/conftest.py)."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_HERE, "../emu"))
import emu_wave  # noqa: E402

_LIB = os.path.join(_HERE, "libqm_probe.so")
_CSRC = os.path.join(_HERE, "../../rapmap_amd/csrc")
_SRC = [os.path.join(_HERE, f) for f in ("qm_probe.hip", "qm_wave_probe.inl", "Makefile")] + \
       [os.path.join(_CSRC, f) for f in ("qm_wave.h", "qm_mapper.inl", "qm_sel.inl", "qm_selpack.inl", "qm_lean.inl", "qm_sweep.h", "qm_lib.inl")] + \
       [os.path.join(_HERE, "../../include/qmap_mi355.h")]
DISPATCH, LOOP, TILES, ONE_TILE = 0, 1, 2, 3                      # `which` of qp_h2m (emu_h2m's numbers)
RING_GMEM = 4096                                                  # the ring whose blocks live in device memory


class ProbeError(RuntimeError):
    pass


def build():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        raise ProbeError("tests/device/libqm_probe.so is missing or older than its sources, and there is no hipcc to build it")
    subprocess.check_call(["make", "-s", "-C", _HERE])


_cached = None
_device_error = None                                              # the first call that came back with a device error: nothing is launched after it
launches = 0                                                      # kernel launches so far (one per call of an entry point)


def _lib():
    global _cached
    if _device_error:
        raise ProbeError("not run: %s failed on the device earlier in this process" % _device_error)
    if _cached is None:
        if not os.path.exists(_LIB) or any(os.path.getmtime(_LIB) < os.path.getmtime(s) for s in _SRC):
            build()
        lib = C.CDLL(_LIB)
        lib.qp_op_name.restype = C.c_char_p
        lib.qp_error_string.restype = C.c_char_p
        _cached = lib
    return _cached


def _check(rc, what):
    global launches, _device_error
    launches += 1
    if rc and rc != 1:                                            # (1: hipErrorInvalidValue, an argument the entry point turned down before launching)
        _device_error = what
    if rc:
        raise ProbeError("%s: hipError_t %d (%s)" % (what, rc, _lib().qp_error_string(C.c_int(rc)).decode()))


def ops():
    lib = _lib()
    return {lib.qp_op_name(i).decode(): i for i in range(lib.qp_n_ops())}


def wave(op, prm, a, b, c, d, mem, atom):
    """W waves of one primitive in one launch (tests/wave_cases.py) -> (out[W, NOUT, 64] uint64, atom[W] uint64)"""
    lib = _lib()
    out, atom, rc = emu_wave.call_wave(lib.qp_wave, ops(), lib.qp_memb(), lib.qp_nout(), op, prm, a, b, c, d, mem, atom)
    _check(rc, "qp_wave(%s)" % op)
    return out, atom


def _fill_two_blocks(cases, least=8):
    """fewer cases than two blocks hold wavefronts: the cases again, in turn, so that each also runs at other places of a block"""
    return list(cases) + [cases[i % len(cases)] for i in range(max(0, least - len(cases)))]


def _first_copies(res, n, what):
    """the answers of the n cases themselves -- their further copies (_fill_two_blocks) must have got the same"""
    for i in range(n, len(res)):
        same = all(np.array_equal(x, y) for x, y in zip(res[i], res[i % n]))
        if not same:
            raise ProbeError("%s: case %d gives another answer in wavefront %d of its block than in wavefront %d" % (what, i % n, i % 4, (i % n) % 4))
    return res[:n]


def tile_range():
    return _lib().qp_h2m_tile_lo(), _lib().qp_h2m_tile_hi()


def h2m_many(which, cases):
    """cases: [(stash (n, 4) uint32 rows {tid, pos, qp, iv}, m, min_idx, is_rc)], one per wavefront of ONE launch; the slots of a wave's stash from n
    on hold 0xA5 -> [(count, elem[64] uint64, keep[64] bool, slot[64] int32)]"""
    asked, cases = len(cases), _fill_two_blocks(cases)
    nw = len(cases)
    hdr = np.zeros((nw, 4), dtype=np.int32)
    stash = np.full((nw, 64, 4), 0xA5A5A5A5, dtype=np.uint32)
    for i, (st, m, min_idx, is_rc) in enumerate(cases):
        st = np.ascontiguousarray(st, dtype=np.uint32).reshape(-1, 4)
        if len(st) > 64:
            raise ValueError("qp_h2m: a stash holds at most 64 suffixes")
        hdr[i] = (len(st), m, min_idx, 1 if is_rc else 0)
        stash[i, :len(st)] = st
    cnt = np.zeros(nw, dtype=np.int32); elem = np.zeros((nw, 64), dtype=np.uint64); keep = np.zeros((nw, 64), dtype=np.uint8); slot = np.zeros((nw, 64), dtype=np.int32)
    rc = _lib().qp_h2m(C.c_int(which), C.c_int(nw), C.c_void_p(hdr.ctypes.data), C.c_void_p(stash.ctypes.data), C.c_void_p(cnt.ctypes.data),
                       C.c_void_p(elem.ctypes.data), C.c_void_p(keep.ctypes.data), C.c_void_p(slot.ctypes.data))
    _check(rc, "qp_h2m(which %d, %d waves)" % (which, nw))
    return _first_copies([(int(cnt[i]), elem[i], keep[i].astype(bool), slot[i]) for i in range(nw)], asked, "qp_h2m")


def _pack(seqs):
    """code strings -> (one byte array, the offset of each)"""
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    buf = np.concatenate([np.asarray(s, dtype=np.uint8) for s in seqs] + [np.zeros(1, dtype=np.uint8)])
    return np.ascontiguousarray(buf), off


def ring_slots(w):
    return _lib().qp_ksw_ring_slots(C.c_int(w))


def ksw_rows(groups, scheme, ring=-1):
    """groups: [[(query, target) x 1 .. 4]] (nt4 code arrays), one group per wavefront of ONE launch, the rows a group leaves out idle; scheme: (match,
    mismatch, gap open, gap extend, band); ring: 32 / 64 / 128 / 1024 slots in LDS, 4096 in device memory, < 0: what the launch wrapper picks for the band
    -> [[score per alignment of the group]]"""
    a, b, q_, e_, w = scheme
    if ring < 0:
        ring = ring_slots(w)
    asked, groups = len(groups), _fill_two_blocks(groups)
    nw = len(groups)
    buf, off = _pack([s for g in groups for qt in g for s in qt])
    hdr = np.zeros((nw, 4, 4), dtype=np.int32)
    k = 0
    for i, g in enumerate(groups):
        assert 1 <= len(g) <= 4
        for r, (qq, tt) in enumerate(g):
            hdr[i, r] = (len(qq), len(tt), off[k], off[k + 1]); k += 2
    out = np.zeros((nw, 4), dtype=np.int32)
    rc = _lib().qp_ksw_rows(C.c_int(ring), C.c_int(nw), C.c_void_p(hdr.ctypes.data), C.c_void_p(buf.ctypes.data), C.c_longlong(len(buf)),
                            C.c_int(a), C.c_int(b), C.c_int(q_), C.c_int(e_), C.c_int(w), C.c_void_p(out.ctypes.data))
    _check(rc, "qp_ksw_rows(ring %d, %d waves, scheme %r)" % (ring, nw, scheme))
    return _first_copies([[int(x) for x in out[i, :len(g)]] for i, g in enumerate(groups)], asked, "qp_ksw_rows")


def sel_side(G, batch, policy, scheme):
    """every question of the batch (tests/sel_side_cases.py: Batch) through sel_side_score<G> in ONE launch, G = 2 / 4 / 8 / 16 lanes per question
    -> (kind[n] int32, tsc[n] int32, key[n] uint64, task[n, 9] int64 rows of emu_sel.TASK_FIELDS) -- what emu_sel.sel_side(.., strip=False) gives"""
    import emu_sel
    reads, roffs, text, txp_off, txp_len, qd = emu_sel.flat(batch)
    n = len(qd)
    prm = np.array([policy] + list(scheme), dtype=np.int32)
    kind = np.zeros(n, dtype=np.int32); tsc = np.zeros(n, dtype=np.int32); key = np.zeros(n, dtype=np.uint64); task = np.zeros((n, 9), dtype=np.int64)
    rc = _lib().qp_sel_side(C.c_int(G), C.c_int(n), C.c_void_p(reads.ctypes.data), C.c_void_p(roffs.ctypes.data), C.c_void_p(text.ctypes.data),
                            C.c_longlong(len(text)), C.c_int(len(txp_off)), C.c_void_p(txp_off.ctypes.data), C.c_void_p(txp_len.ctypes.data),
                            C.c_void_p(qd.ctypes.data), C.c_void_p(prm.ctypes.data), C.c_void_p(kind.ctypes.data), C.c_void_p(tsc.ctypes.data),
                            C.c_void_p(key.ctypes.data), C.c_void_p(task.ctypes.data))
    _check(rc, "qp_sel_side(%d lanes, %d questions, policy %d, scheme %r)" % (G, n, policy, scheme))
    return kind, tsc, key, task


def sel_strip(tasks, batch, scheme):
    """tasks: (n, 9) rows of emu_sel.TASK_FIELDS as sel_side leaves them for the questions with kind & 4, run four per wavefront in this order in ONE
    launch of sel_tasks_strip -> scores[n] int32"""
    import emu_sel
    reads, roffs, text, txp_off, txp_len, qd = emu_sel.flat(batch)
    t = np.ascontiguousarray(np.asarray(tasks, dtype=np.int64)[:, [1, 4, 5, 6, 2, 7, 8]])       # {read offset, rl, roff, rlen, target offset, tlen1, fwd}
    n = len(t)
    prm = np.array(scheme[:4], dtype=np.int32)
    out = np.zeros(n, dtype=np.int32)
    rc = _lib().qp_sel_strip(C.c_int(n), C.c_void_p(t.ctypes.data), C.c_void_p(reads.ctypes.data), C.c_longlong(len(reads)), C.c_void_p(text.ctypes.data),
                             C.c_longlong(len(text)), C.c_void_p(prm.ctypes.data), C.c_void_p(out.ctypes.data))
    _check(rc, "qp_sel_strip(%d alignments, scheme %r)" % (n, scheme))
    return out


def ksw_rows8(groups, scheme):
    """groups: [[(query, target) x 1 .. 8]], every alignment of a group of one shape, one group per wavefront of ONE launch -> [[score per alignment]]"""
    a, b, q_, e_, w = scheme
    asked, groups = len(groups), _fill_two_blocks(groups)
    nw = len(groups)
    buf, off = _pack([s for g in groups for qt in g for s in qt])
    hdr = np.zeros((nw, 20), dtype=np.int32)
    k = 0
    for i, g in enumerate(groups):
        assert 1 <= len(g) <= 8 and all(len(qq) == len(g[0][0]) and len(tt) == len(g[0][1]) for qq, tt in g)
        hdr[i, :3] = (len(g), len(g[0][0]), len(g[0][1]))
        for r in range(len(g)):
            hdr[i, 4 + 2 * r], hdr[i, 5 + 2 * r] = off[k], off[k + 1]; k += 2
    out = np.zeros((nw, 8), dtype=np.int32)
    rc = _lib().qp_ksw_rows8(C.c_int(nw), C.c_void_p(hdr.ctypes.data), C.c_void_p(buf.ctypes.data), C.c_longlong(len(buf)),
                             C.c_int(a), C.c_int(b), C.c_int(q_), C.c_int(e_), C.c_int(w), C.c_void_p(out.ctypes.data))
    _check(rc, "qp_ksw_rows8(%d waves, scheme %r)" % (nw, scheme))
    return _first_copies([[int(x) for x in out[i, :len(g)]] for i, g in enumerate(groups)], asked, "qp_ksw_rows8")
