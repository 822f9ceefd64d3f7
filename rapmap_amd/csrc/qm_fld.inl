// qm_fld.inl -- the fragment-length histogram: the hit lists of a mapped batch folded into fragment length -> number of fragments.
//
// Written against qm_wave.h, on the frame of qm_sweep.h: the same source runs lane by lane under -DQM_EMU (tests/emu/qm_emu_fld.cpp).
// fld_wave is the body of ONE wavefront; qx::sweep (qm_exec.h) is its kernel.  Every unit falls into exactly one of six categories
// (the first condition that holds, include/qmap_mi355.h): unmapped, multi, not_paired, same_strand, out_of_range, used.  Only a used
// unit touches a bin.  Integer adds only: the result is the same bits whatever the grid and whatever order the wavefronts arrive in.
//
//   1. the wavefront zeroes the max_len + 1 words of its own LDS slab
//   2. it strides over the units, one lane per unit (unit_bounds); only a lane whose unit has exactly one hit loads from that hit's
//      record -- the dword at byte 12 (frag_len) and the dword at byte 24 (fwd, mate_is_fwd, is_paired, mate_status), one 32-byte
//      sector -- so a batch without hits never touches the hit buffer; the categories are ballots and popcounts on the scalar
//      unit (frag_gate, tally), a used lane adds one to its bin in the slab (an LDS integer atomic)
//   3. the flush: the slab's non-zero bins go out by integer atomics on the 64-bit global bins, then the six counters, at most one
//      atomic each per wavefront
#pragma once
#include "qm_sweep.h"

namespace qm {

static_assert(sizeof(qm_hit) == 32 && offsetof(qm_hit, frag_len) == 12 && offsetof(qm_hit, fwd) == 24 && offsetof(qm_hit, mate_is_fwd) == 25 &&
              offsetof(qm_hit, is_paired) == 26 && offsetof(qm_hit, mate_status) == 27, "fld_wave reads a hit record's dwords at bytes 12 and 24");

#define FLD_SLAB 1024        // words of a wavefront's LDS slab: max_len + 1 <= 1024 bins of 4 bytes, 4 KB; and of the object's 64-bit bins
// workgroups resident per compute unit: 8 waves per SIMD = 32 per CU = 8 workgroups (16 KB of LDS each: 128 of the CU's 160 KB)
#define FLD_BLOCKS_PER_CU 8
enum { FLD_C_WORDS = SW_C_WORDS };   // the object's counter words behind its bins: the frame's, none of its own

#ifdef QM_EMU
QM_DEV void fld_load_rec(const unsigned char* r, u32& f, u32& w) { f = *(const u32*)(r + 12); w = *(const u32*)(r + 24); }
#else
// the record's two dwords, both loads in flight before either is looked at (see load_32 in qm_wave.h)
QM_DEV void fld_load_rec(const unsigned char* r, u32& f, u32& w) {
  u32 a = *(const u32*)(r + 12), b = *(const u32*)(r + 24);
  asm volatile("" : "+v"(a), "+v"(b));
  f = a; w = b;
}
#endif

// wavefront `wave` of `nWaves` (both wave-uniform); slab: FLD_SLAB words of its own
QM_DEV void fld_wave(const UnitSrc& S, const SweepAcc& A, long long wave, long long nWaves, QM_LDS(u32)* slab) {
  const int nb = A.maxLen + 1;
  slab_zero(slab, nb);
  u64 ctr[SW_C_GATE] = {0, 0, 0, 0, 0, 0};
  for (long long base = wave * 64; base < S.n; base += nWaves * 64) {
    LV<long long> o0, o1;
    unit_bounds(S, base, o0, o1);
    LV<int> cat; LV<u32> fl;
    QM_LANES(l) {
      cat[l] = -1; fl[l] = 0;
      if (base + l >= S.n) continue;
      const long long c = o1[l] - o0[l];
      u32 f = 0, w = 0;
      if (c == 1) fld_load_rec(S.hits + o0[l] * (long long)S.stride, f, w);
      cat[l] = frag_gate(c, f, w, A.maxLen); fl[l] = f;
    }
    tally<SW_C_GATE>(cat, ctr);
    QM_LANES(l) if (cat[l] == SW_C_USED) slab_inc(slab + fl[l]);
  }
  slab_flush(slab, nb, A.bins);
  const int word[SW_C_GATE] = {SW_C_USED, SW_C_UNMAPPED, SW_C_MULTI, SW_C_NOT_PAIRED, SW_C_SAME_STRAND, SW_C_OUT_OF_RANGE};
  flush_counters(A.ctr, ctr, word);
}

}  // namespace qm
