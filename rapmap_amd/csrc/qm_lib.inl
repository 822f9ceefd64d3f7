// qm_lib.inl -- the library type: the hit records of a mapped batch classified by orientation, tallied, and the hits whose code a
// library type keeps compacted into plain tid lists for the equivalence-class fold.
//
// Written against qm_wave.h: the same source runs lane by lane under -DQM_EMU (tests/emu/qm_emu_lib.cpp).  Every function here is
// the body of ONE wavefront.  A hit's CODE (include/qmap_mi355.h, the table there) comes from one function, lib_hit_code; a library
// type is a 12-bit mask over the codes.  Integer adds only: the tallies are the same bits whatever the grid and whatever order the
// wavefronts arrive in; there is no floating point.
//
//   lib_classify_wave   a persistent grid, one lane per HIT (not per unit: the loads coalesce and a unit of 2 000 hits is nothing
//                       special): hit wavefront w = hits [64 w, 64 w + 64).  Every lane loads the dwords at bytes 4, 8 and 24 of
//                       its record, all three in flight before any is looked at; the twelve codes, `other` and "kept" are ballots,
//                       their popcounts wave-uniform accumulators; the keep ballot goes out as keepMask[w], its popcount as
//                       keepCnt[w]: 12 bytes of scratch per 64 hits.  At its end a wavefront flushes its non-zero accumulators, at
//                       most one integer atomic per counter and wavefront.
//   (the host scans keepCnt into waveBase)
//   lib_compact_wave    lane l of hit wavefront w writes its tid to outTids[waveBase[w] + popc(keepMask[w] & lanemask_lt(l))]
//                       when its bit is set: the kept hits in their order
//   lib_units_wave      a persistent grid, one lane per unit, on the frame of qm_sweep.h: with P(h) = waveBase[h >> 6] +
//                       popc(keepMask[h >> 6] & bits below h & 63), newOff[u] = P(off[u]); off[u + 1] is loaded once and P of it
//                       computed once, off[u] and its P come from the lane below (unit_bounds, lane_below_i64).  Units, unmapped,
//                       kept and dropped are ballots; a unit of exactly one hit derives that hit's code again for the single-hit
//                       words.
// Both persistent grids are launched by qx::sweep (qm_exec.h).  The classify pass is a sweep over HITS and has no sibling: of the
// frame it shares the tails (tally, flush_counters).
#pragma once
#include "qm_sweep.h"

namespace qm {

static_assert(sizeof(qm_hit) == 32 && offsetof(qm_hit, tid) == 0 && offsetof(qm_hit, pos) == 4 && offsetof(qm_hit, mate_pos) == 8 && offsetof(qm_hit, fwd) == 24 &&
              offsetof(qm_hit, mate_is_fwd) == 25 && offsetof(qm_hit, mate_status) == 27, "the library-type sweep reads a hit record's dwords at bytes 0, 4, 8 and 24");

enum { LIB_ISF = 0, LIB_ISR = 1, LIB_OSF = 2, LIB_OSR = 3, LIB_MSF = 4, LIB_MSR = 5, LIB_LF = 6, LIB_LR = 7, LIB_RF = 8, LIB_RR = 9, LIB_SF = 10, LIB_SR = 11,
       LIB_CODES = 12, LIB_OTHER = 12 };
// the 32 words of a tally (include/qmap_mi355.h)
enum { LIB_W_HITS_BY_CODE = 0, LIB_W_SINGLE_BY_CODE = 12, LIB_W_UNITS = 24, LIB_W_UNMAPPED = 25, LIB_W_KEPT_UNITS = 26, LIB_W_DROPPED_UNITS = 27,
       LIB_W_HITS = 28, LIB_W_KEPT_HITS = 29, LIB_W_OTHER_HITS = 30, LIB_WORDS = 32 };
#define LIB_ALL_CODES 0xfffu
// workgroups of the two persistent kernels resident per compute unit: 8 waves per SIMD = 32 per CU = 8 workgroups
#define LIB_BLOCKS_PER_CU 8

typedef UnitSrc LibSrc;      // the units of a sweep, under the name the sweep's callers give them
struct LibAcc {
  u64* ctr;                  // [LIB_WORDS]
  u32 mask;                  // the codes kept
  u64* keepMask; u32* keepCnt; long long* waveBase;   // per hit wavefront (waveBase: one entry more, the total)
  u32* outTids; long long* newOff;                     // the kept hits' tids and the units' offsets into them ([n + 1]); null: not wanted
};

// the code of a hit record from its pos, mate_pos and the dword at byte 24 (fwd, mate_is_fwd, is_paired, mate_status); a byte
// counts as forward when it is not 0.  Outward is the reference's dovetail predicate, compared as signed numbers.
QM_DEV int lib_hit_code(int pos, int matePos, u32 w) {
  const bool f = (w & 0xffu) != 0, mf = ((w >> 8) & 0xffu) != 0;
  const u32 ms = w >> 24;
  if (ms == 3u) {
    if (f == mf) return f ? LIB_MSF : LIB_MSR;
    const bool outward = (f && pos > matePos) || (mf && matePos > pos);
    return (outward ? LIB_OSF : LIB_ISF) + (f ? 0 : 1);
  }
  if (ms > 3u) return LIB_OTHER;
  return (ms == 1u ? LIB_LF : ms == 2u ? LIB_RF : LIB_SF) + (f ? 0 : 1);
}

#ifdef QM_EMU
QM_DEV void lib_load_rec(const unsigned char* r, int& pos, int& matePos, u32& w) { pos = *(const int*)(r + 4); matePos = *(const int*)(r + 8); w = *(const u32*)(r + 24); }
#else
// the record's three dwords, all loads in flight before any is looked at (see fld_load_rec)
QM_DEV void lib_load_rec(const unsigned char* r, int& pos, int& matePos, u32& w) {
  int a = *(const int*)(r + 4), b = *(const int*)(r + 8); u32 c = *(const u32*)(r + 24);
  asm volatile("" : "+v"(a), "+v"(b), "+v"(c));
  pos = a; matePos = b; w = c;
}
#endif

// the words of the classify sweep's fifteen accumulators (the twelve codes, other, kept hits, hits) and of the unit sweep's sixteen
// (the twelve single-hit codes, units, unmapped, kept, dropped)
#define LIB_CLASSIFY_WORDS {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, LIB_W_OTHER_HITS, LIB_W_KEPT_HITS, LIB_W_HITS}
#define LIB_UNITS_WORDS {12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, LIB_W_UNITS, LIB_W_UNMAPPED, LIB_W_KEPT_UNITS, LIB_W_DROPPED_UNITS}
static_assert(LIB_W_HITS_BY_CODE == 0 && LIB_W_SINGLE_BY_CODE == 12 && LIB_CODES == 12, "the first twelve words of both maps");

// wavefront `wave` of `nWaves` (both wave-uniform) over the hit wavefronts
QM_DEV void lib_classify_wave(const UnitSrc& S, const LibAcc& A, long long wave, long long nWaves) {
  u64 acc[15];               // the twelve codes, other, kept hits, hits
#pragma unroll
  for (int i = 0; i < 15; ++i) acc[i] = 0;
  const long long hw = (S.nh + 63) >> 6;
  for (long long w = wave; w < hw; w += nWaves) {
    LV<int> code; LV<bool> b;
    QM_LANES(l) {
      const long long h = w * 64 + l;
      code[l] = -1;
      if (h < S.nh) {
        int pos, matePos; u32 wd;
        lib_load_rec(S.hits + h * (long long)S.stride, pos, matePos, wd);
        code[l] = lib_hit_code(pos, matePos, wd);
      }
    }
    tally<LIB_OTHER + 1>(code, acc);
    QM_LANES(l) b[l] = code[l] >= 0 && code[l] < LIB_CODES && ((A.mask >> code[l]) & 1u);
    const u64 keep = ballot(b);
    QM_LANES(l) b[l] = code[l] >= 0;
    acc[13] += (u64)popc64(keep); acc[14] += (u64)popc64(ballot(b));
    QM_LANES(l) if (l == 0) { A.keepMask[w] = keep; A.keepCnt[w] = (u32)popc64(keep); }
  }
  const int word[15] = LIB_CLASSIFY_WORDS;
  flush_counters(A.ctr, acc, word);
}

// hit wavefront `wave`: the kept hits' tids, in their order
QM_DEV void lib_compact_wave(const UnitSrc& S, const LibAcc& A, long long wave) {
  const u64 keep = uniform(A.keepMask[wave]);
  if (!keep) return;
  const long long base = load_uniform_i64(A.waveBase + wave);
  QM_LANES(l) {
    const long long h = wave * 64 + l;
    if (h < S.nh && ((keep >> l) & 1)) A.outTids[base + popc64(keep & lanemask_lt(l))] = *(const u32*)(S.hits + h * (long long)S.stride);
  }
}

// kept hits in front of hit h (0 <= h <= nh); the word of a hit wavefront that does not exist is never read
QM_DEV long long lib_kept_before(const LibAcc& A, long long h) {
  const int r = (int)(h & 63);
  return A.waveBase[h >> 6] + (r ? popc64(A.keepMask[h >> 6] & lanemask_lt(r)) : 0);
}

// wavefront `wave` of `nWaves` (both wave-uniform) over the units, one lane per unit
QM_DEV void lib_units_wave(const UnitSrc& S, const LibAcc& A, long long wave, long long nWaves) {
  u64 acc[16];               // the twelve single-hit codes, units, unmapped, kept, dropped
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0;
  for (long long base = wave * 64; base < S.n; base += nWaves * 64) {
    LV<long long> o0, o1, p0, p1;                               // the unit's bounds and the kept hits in front of each
    const long long first = unit_bounds(S, base, o0, o1);
    QM_LANES(l) p1[l] = base + l < S.n ? lib_kept_before(A, o1[l]) : 0;
    lane_below_i64(p1, lib_kept_before(A, first), p0);
    LV<int> code, what; LV<bool> valid;                         // what: 0 unmapped, 1 a unit with kept hits, 2 dropped
    QM_LANES(l) {
      code[l] = what[l] = -1;
      const long long u = base + l;
      valid[l] = u < S.n;
      if (!valid[l]) continue;
      if (A.newOff) { A.newOff[u + 1] = p1[l]; if (u == 0) A.newOff[0] = p0[l]; }
      const long long c = o1[l] - o0[l];
      what[l] = c == 0 ? 0 : p1[l] > p0[l] ? 1 : 2;
      if (c == 1) {
        int pos, matePos; u32 wd;
        lib_load_rec(S.hits + o0[l] * (long long)S.stride, pos, matePos, wd);
        code[l] = lib_hit_code(pos, matePos, wd);
      }
    }
    tally<LIB_CODES>(code, acc);
    acc[12] += (u64)popc64(ballot(valid));
    tally<3>(what, acc + 13);
  }
  const int word[16] = LIB_UNITS_WORDS;
  flush_counters(A.ctr, acc, word);
}

}  // namespace qm
