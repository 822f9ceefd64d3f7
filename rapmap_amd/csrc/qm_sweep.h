// qm_sweep.h -- the frame of a per-batch tally: what every sweep over the units of a mapped batch does the same way, once.
//
// Written against qm_wave.h: the same source runs lane by lane under -DQM_EMU (tests/emu).  A sweep is a persistent grid (qx::sweep,
// qm_exec.h) whose wavefronts stride over the units, one lane per unit, count into wave-uniform accumulators and, where it has
// bins, into an LDS slab of the wavefront's own; at its end a wavefront flushes both with integer atomics, so the result is the
// same bits whatever the grid.  The pieces (held to a numpy restatement one by one: tests/wave_cases.py):
//
//   UnitSrc, SweepAcc     what a sweep reads and where a tally with bins adds to
//   lane_below_i64        every lane gets a 64-bit value of the lane below
//   unit_bounds           (off[u], off[u + 1]) per lane from ONE coalesced load
//   frag_gate, tally      the category of a unit as a fragment, and the categories counted by ballots
//   slab_zero / slab_inc / slab_flush, flush_counters     the bins in LDS and the tails
//
// What differs between the sweeps stays with them: the record loader (2, 3 or 5 dwords on purpose) and the bin rule.
#pragma once
#include <stddef.h>
#include "qm_wave.h"
#include "../../include/qmap_mi355.h"

namespace qm {

struct UnitSrc {             // the units of a batch
  const unsigned char* hits; int stride;   // hit j's record: hits + j * stride (32: qm_hit); may be null when no unit has a hit
  const long long* off;      // [n + 1]
  long long n, nh;           // units, hits (= off[n] - off[0])
};
struct SweepAcc {            // a tally with bins, as it lies in device memory
  u64* bins;                 // [at least maxLen + 1, or the sweep's own number]
  u64* ctr;                  // [SW_C_WORDS]
  int maxLen;
};

// the categories of a unit as a fragment, the first that holds (include/qmap_mi355.h); they are the counter words of a tally with
// bins.  Word SW_C_GATE is the first a sweep may add a category of its own to (the GC sweep: overhang).
enum { SW_C_USED = 0, SW_C_UNMAPPED = 1, SW_C_MULTI = 2, SW_C_NOT_PAIRED = 3, SW_C_SAME_STRAND = 4, SW_C_OUT_OF_RANGE = 5, SW_C_GATE = 6, SW_C_WORDS = 8 };

// out[l] = x[l - 1]; lane 0 has no lane below and takes `first` (wave-uniform).  All 64 lanes active.  A 64-bit value travels as
// its two dwords, one DPP move each.
QM_DEV void lane_below_i64(const LV<long long>& x, long long first, LV<long long>& out) {
  LV<int> lo, hi, loB, hiB;
  QM_LANES(l) { lo[l] = (int)(u32)(u64)x[l]; hi[l] = (int)(u32)((u64)x[l] >> 32); }
  lane_rotate_up(lo, loB); lane_rotate_up(hi, hiB);
  QM_LANES(l) out[l] = l ? (long long)(((u64)(u32)hiB[l] << 32) | (u32)loB[l]) : first;
}

// lane l: o0 = off[base + l], o1 = off[base + l + 1] -- off[u + 1] from one coalesced 8-byte load per lane, off[u] from the lane
// below, the first lane's from one wave-uniform load, which is also what comes back (off[base]).  base (wave-uniform) < n; what a
// lane past n gets is not a bound.
QM_DEV long long unit_bounds(const UnitSrc& S, long long base, LV<long long>& o0, LV<long long>& o1) {
  QM_LANES(l) { const long long u = base + l; o1[l] = u < S.n ? S.off[u + 1] : 0; }
  const long long first = load_uniform_i64(S.off + base);
  lane_below_i64(o1, first, o0);
  return first;
}

// the category of a unit of c hits; f, w: frag_len and the dword at byte 24 (fwd, mate_is_fwd, is_paired, mate_status) of its
// record when c == 1 (not looked at otherwise)
QM_DEV int frag_gate(long long c, u32 f, u32 w, int maxLen) {
  if (c == 0) return SW_C_UNMAPPED;
  if (c != 1) return SW_C_MULTI;
  if ((w >> 24) != 3u) return SW_C_NOT_PAIRED;                    // mate_status != PE_PAIRED
  if ((w & 0xffu) == ((w >> 8) & 0xffu)) return SW_C_SAME_STRAND;   // fwd == mate_is_fwd
  if (f == 0 || f > (u32)maxLen) return SW_C_OUT_OF_RANGE;
  return SW_C_USED;
}

// acc[i] += the lanes whose category is i, for i < N (a lane without one: -1): a ballot and a popcount each, on the scalar unit
template <int N>
QM_DEV void tally(const LV<int>& cat, u64* acc) {
  LV<bool> b;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    QM_LANES(l) b[l] = cat[l] == i;
    acc[i] += (u64)popc64(ballot(b));
  }
}

#ifdef QM_EMU
QM_DEV void slab_inc(QM_LDS(u32)* p) { *p += 1; }
#else
// ds_add_u32 without a return value; the slab is this wavefront's own, the lanes of one instruction may share a bin
QM_DEV void slab_inc(QM_LDS(u32)* p) { (void)__hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
#endif
// the first n words of the wavefront's slab zeroed (a slab arrives with anything in it) ...
QM_DEV void slab_zero(QM_LDS(u32)* slab, int n) {
  QM_LANES(l) for (int i = l; i < n; i += 64) slab[i] = 0;
  wave_fence();
}
// ... and at the end its non-zero words added to the 64-bit bins
QM_DEV void slab_flush(const QM_LDS(u32)* slab, int n, u64* bins) {
  wave_fence();
  QM_LANES(l) for (int i = l; i < n; i += 64) { const u32 v = slab[i]; if (v) atomic_add_u64(&bins[i], (u64)v); }
}

// lane i (< N <= 64) adds accumulator i to ctr[word[i]] when it is not 0: at most one atomic per counter and wavefront
template <int N>
QM_DEV void flush_counters(u64* ctr, const u64 (&acc)[N], const int (&word)[N]) {
  static_assert(N <= 64, "a lane per accumulator");
  QM_LANES(l) {
    u64 v = 0; int w = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) if (l == i) { v = acc[i]; w = word[i]; }
    if (v) atomic_add_u64(&ctr[w], v);
  }
}

}  // namespace qm
