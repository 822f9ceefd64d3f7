// qm_fld.inl -- the fragment-length histogram: the hit lists of a mapped batch folded into fragment length -> number of fragments.
//
// Written against qm_wave.h: the same source runs lane by lane under -DQM_EMU (tests/emu/qm_emu_fld.cpp).  fld_wave is the body of
// ONE wavefront; qm_kernels_fld.hip wraps it into the kernel.  Every unit falls into exactly one of six categories (the first
// condition that holds, include/qmap_mi355.h): unmapped, multi, not_paired, same_strand, out_of_range, used.  Only a used unit
// touches a bin.  Integer adds only: the result is the same bits whatever the grid and whatever order the wavefronts arrive in.
//
//   1. the wavefront zeroes the max_len + 1 words of its own LDS slab
//   2. it strides over the units, one lane per unit: off[u + 1] comes from one coalesced 8-byte load per lane, off[u] from the lane
//      below (the first lane's: one wave-uniform load); only a lane whose unit has exactly one hit loads from that hit's record --
//      the dword at byte 12 (frag_len) and the dword at byte 24 (fwd, mate_is_fwd, is_paired, mate_status), one 32-byte sector --
//      so a batch without hits never touches the hit buffer; the five other categories are ballots and popcounts on the scalar
//      unit, a used lane adds one to its bin in the slab (an LDS integer atomic)
//   3. the flush: the slab's non-zero bins go out by integer atomics on the 64-bit global bins, then the six counters, at most one
//      atomic each per wavefront
#pragma once
#include <stddef.h>
#include "qm_wave.h"
#include "../../include/qmap_mi355.h"

namespace qm {

static_assert(sizeof(qm_hit) == 32 && offsetof(qm_hit, frag_len) == 12 && offsetof(qm_hit, fwd) == 24 && offsetof(qm_hit, mate_is_fwd) == 25 &&
              offsetof(qm_hit, is_paired) == 26 && offsetof(qm_hit, mate_status) == 27, "fld_wave reads a hit record's dwords at bytes 12 and 24");

#define FLD_SLAB 1024        // words of a wavefront's LDS slab: max_len + 1 <= 1024 bins of 4 bytes, 4 KB
enum { FLD_C_USED = 0, FLD_C_UNMAPPED = 1, FLD_C_MULTI = 2, FLD_C_NOT_PAIRED = 3, FLD_C_SAME_STRAND = 4, FLD_C_OUT_OF_RANGE = 5, FLD_C_WORDS = 8 };
#define FLD_ACC_WORDS (FLD_SLAB + FLD_C_WORDS)   // the object's device memory: the 64-bit bins, then the counters
// workgroups resident per compute unit: 8 waves per SIMD = 32 per CU = 8 workgroups (16 KB of LDS each: 128 of the CU's 160 KB)
#define FLD_BLOCKS_PER_CU 8

struct FldSrc {              // the units of a fold
  const unsigned char* hits; int stride;   // hit j's record: hits + j * stride (32: qm_hit); may be null when no unit has a hit
  const long long* off;      // [n + 1]
  long long n;
};
struct FldAcc {
  u64* bins;                 // [maxLen + 1]
  u64* ctr;                  // [FLD_C_WORDS]
  int maxLen;
};

#ifdef QM_EMU
QM_DEV void fld_slab_inc(QM_LDS(u32)* p) { *p += 1; }
QM_DEV void fld_load_rec(const unsigned char* r, u32& f, u32& w) { f = *(const u32*)(r + 12); w = *(const u32*)(r + 24); }
#else
// the record's two dwords, both loads in flight before either is looked at (see load_32 in qm_wave.h)
QM_DEV void fld_load_rec(const unsigned char* r, u32& f, u32& w) {
  u32 a = *(const u32*)(r + 12), b = *(const u32*)(r + 24);
  asm volatile("" : "+v"(a), "+v"(b));
  f = a; w = b;
}
// ds_add_u32 without a return value; the slab is this wavefront's own, the lanes of one instruction may share a bin
QM_DEV void fld_slab_inc(QM_LDS(u32)* p) { (void)__hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
#endif

// wavefront `wave` of `nWaves` (both wave-uniform); slab: FLD_SLAB words of its own
QM_DEV void fld_wave(const FldSrc& S, const FldAcc& A, long long wave, long long nWaves, QM_LDS(u32)* slab) {
  const int nb = A.maxLen + 1;
  QM_LANES(l) for (int i = l; i < nb; i += 64) slab[i] = 0;
  wave_fence();
  u64 ctr[6] = {0, 0, 0, 0, 0, 0};
  for (long long base = wave * 64; base < S.n; base += nWaves * 64) {
    LV<int> hiLo, hiHi, loLo, loHi;                             // off[u + 1] as two dwords, and the lane below's
    QM_LANES(l) {
      const long long u = base + l;
      const long long e = u < S.n ? S.off[u + 1] : 0;
      hiLo[l] = (int)(u32)(u64)e; hiHi[l] = (int)(u32)((u64)e >> 32);
    }
    lane_rotate_up(hiLo, loLo); lane_rotate_up(hiHi, loHi);
    const long long first = load_uniform_i64(S.off + base);     // off[base]: lane 0 has no lane below
    LV<bool> unm, multi, np, ss, oor, used; LV<u32> fl;
    QM_LANES(l) {
      unm[l] = multi[l] = np[l] = ss[l] = oor[l] = used[l] = false; fl[l] = 0;
      const long long u = base + l;
      if (u >= S.n) continue;
      const long long o1 = (long long)(((u64)(u32)hiHi[l] << 32) | (u32)hiLo[l]);
      const long long o0 = l ? (long long)(((u64)(u32)loHi[l] << 32) | (u32)loLo[l]) : first;
      const long long c = o1 - o0;
      if (c == 0) unm[l] = true;
      else if (c != 1) multi[l] = true;
      else {
        const unsigned char* r = S.hits + o0 * (long long)S.stride;
        u32 f, w;
        fld_load_rec(r, f, w);
        if ((w >> 24) != 3u) np[l] = true;                      // mate_status != PE_PAIRED
        else if ((w & 0xffu) == ((w >> 8) & 0xffu)) ss[l] = true;   // fwd == mate_is_fwd
        else if (f == 0 || f > (u32)A.maxLen) oor[l] = true;
        else { used[l] = true; fl[l] = f; }
      }
    }
    ctr[FLD_C_UNMAPPED] += (u64)popc64(ballot(unm)); ctr[FLD_C_MULTI] += (u64)popc64(ballot(multi)); ctr[FLD_C_NOT_PAIRED] += (u64)popc64(ballot(np));
    ctr[FLD_C_SAME_STRAND] += (u64)popc64(ballot(ss)); ctr[FLD_C_OUT_OF_RANGE] += (u64)popc64(ballot(oor)); ctr[FLD_C_USED] += (u64)popc64(ballot(used));
    QM_LANES(l) if (used[l]) fld_slab_inc(slab + fl[l]);
  }
  wave_fence();
  QM_LANES(l) for (int i = l; i < nb; i += 64) { const u32 v = slab[i]; if (v) atomic_add_u64(&A.bins[i], (u64)v); }
  // the counter flush: lane i holds counter i
  QM_LANES(l) {
    if (l >= 6) continue;
    const u64 v = l == 0 ? ctr[0] : l == 1 ? ctr[1] : l == 2 ? ctr[2] : l == 3 ? ctr[3] : l == 4 ? ctr[4] : ctr[5];
    if (v) atomic_add_u64(&A.ctr[l], v);
  }
}

}  // namespace qm
