// qm_gcb.inl -- fragment GC bias: the GC rank structure over the transcript text, the observed histogram (the fragments of a mapped
// batch by the GC fraction of their window on the transcript) and the expected matrix (the same count over every window a fragment
// could have come from).  The model is in include/qmap_mi355.h; integers only.
//
// Written against qm_wave.h: the same source runs lane by lane under -DQM_EMU (tests/emu/qm_emu_gcb.cpp).  Every function here is the
// body of ONE wavefront.  Integer ballots, adds and atomics only: a result is the same bits whatever the grid and whatever order
// the wavefronts arrive in.
//
// The rank structure: one 64-bit mask per 64 text characters (bit i: character 64 b + i is G, C, g or c) and, per block, the number
// of GC characters in front of it (32 bits: the text has fewer than 2^32 characters).  GC of text positions [a, b) is
// rank_at(b) - rank_at(a), a popcount each.  The structure has (n + 63) / 64 + 2 blocks: the blocks behind the text are empty, so
// the expected kernel's look-ahead word and rank_at(n) need no bound check.
//
//   gcb_mask_wave    64 blocks per wavefront: a ballot per block, lane j keeps block j's, then one coalesced store of masks and counts
//   gcb_rank_wave    the exclusive scan of the counts (64-bit, qx::scan_u32) narrowed to 32 bits
//   gcb_probe_wave   qm_gcb_window_gc: one lane per question
//   gcb_obs_wave     the observed sweep, on the frame of qm_sweep.h (below)
//   gcb_tiles_wave   tiles (GCB_TILE consecutive starts) per transcript, for the scan that gives the tile table
//   gcb_expect_wave  the expected matrix: a persistent grid, launched by qx::sweep like the observed sweep (below)
#pragma once
#include <stddef.h>
#include "qm_sweep.h"

namespace qm {

static_assert(sizeof(qm_hit) == 32 && offsetof(qm_hit, tid) == 0 && offsetof(qm_hit, pos) == 4 && offsetof(qm_hit, mate_pos) == 8 &&
              offsetof(qm_hit, frag_len) == 12 && offsetof(qm_hit, fwd) == 24 && offsetof(qm_hit, mate_is_fwd) == 25 &&
              offsetof(qm_hit, is_paired) == 26 && offsetof(qm_hit, mate_status) == 27,
              "gcb_obs_wave reads a hit record's 16 bytes at 0 and the dword at byte 24: one 32-byte sector");

#define GCB_BINS QM_GCB_BINS
#define GCB_SLAB 32          // words of a wavefront's LDS tally, and of the object's 64-bit bins in device memory
#define GCB_BLOCKS_PER_CU 8  // workgroups of four wavefronts resident per compute unit (both sweeps)
#define GCB_TILE 64          // consecutive start positions of one transcript: one lane each
#define GCB_MAX_LEN 1023     // the longest fragment: g * 2 * GCB_BINS < 2^16 and the reciprocal rule below hold up to here

static_assert(GCB_BINS <= GCB_SLAB && GCB_BINS <= 64 && GCB_MAX_LEN * 2 * GCB_BINS < (1 << 16), "bins: a lane each; the bin rule's range");

inline long long gcb_blocks(long long n) { return (n + 63) / 64 + 2; }   // (host: the drivers size the structure)

struct GcbIdx {              // the rank structure and the transcripts, as they lie in the replica
  const u64* mask; const u32* rank;      // [gcb_blocks(n)]
  const u32* txpOff; const int* txpLen;  // [nTxp]
  long long nTxp, n;
};

QM_DEV bool gcb_is_gc(unsigned c) { c |= 0x20u; return c == 'g' || c == 'c'; }
// GC characters in text positions [0, p), p <= n
QM_DEV u32 gcb_rank_at(const GcbIdx& I, long long p) {
  const long long b = p >> 6;
  return I.rank[b] + (u32)popc64(I.mask[b] & lanemask_lt((int)(p & 63)));
}
// min(NB - 1, (g * NB) / n), n >= 1
QM_DEV u32 gcb_bin(u32 g, u32 n) { const u32 q = g * GCB_BINS / n; return q < GCB_BINS - 1 ? q : GCB_BINS - 1; }

QM_DEV void gcb_mask_wave(const unsigned char* text, long long n, long long nBlk, u64* mask, u32* cnt, long long wave) {
  LV<u64> keep;
  QM_LANES(l) keep[l] = 0;
  for (int j = 0; j < 64; ++j) {
    const long long b = wave * 64 + j;
    if (b >= nBlk) break;
    LV<bool> gc;
    QM_LANES(l) { const long long p = b * 64 + l; gc[l] = p < n && gcb_is_gc(text[p]); }
    const u64 m = ballot(gc);
    QM_LANES(l) if (l == j) keep[l] = m;
  }
  QM_LANES(l) {
    const long long b = wave * 64 + l;
    if (b < nBlk) { mask[b] = keep[l]; cnt[b] = (u32)popc64(keep[l]); }
  }
}

QM_DEV void gcb_rank_wave(const long long* scan, long long nBlk, u32* rank, long long wave) {
  QM_LANES(l) { const long long b = wave * 64 + l; if (b < nBlk) rank[b] = (u32)scan[b]; }
}

// out[i] = GC characters of transcript tid[i] in [start[i], start[i] + len[i]); -1 where the window is empty or does not lie on the transcript
QM_DEV void gcb_probe_wave(const GcbIdx& I, long long nq, const u32* tid, const int* start, const int* len, int* out, long long wave) {
  QM_LANES(l) {
    const long long i = wave * 64 + l;
    if (i >= nq) continue;
    int r = -1;
    const u32 t = tid[i]; const long long s = start[i], e = s + len[i];
    if ((long long)t < I.nTxp && s >= 0 && len[i] >= 1 && e <= (long long)I.txpLen[t]) {
      const long long o = I.txpOff[t];
      r = (int)(gcb_rank_at(I, o + e) - gcb_rank_at(I, o + s));
    }
    out[i] = r;
  }
}

// ---- the observed sweep, on the frame of qm_sweep.h.  Only a lane whose unit has exactly one hit loads from that hit's record -- 16
// bytes at 0 (tid, pos, mate_pos, frag_len) and the dword at byte 24 (fwd, mate_is_fwd, is_paired, mate_status), one 32-byte sector; a
// lane that passes the categories of the fragment-length histogram (frag_gate) gathers txpOff and txpLen and, where the window lies
// on the transcript, the two rank lookups; where it does not, the unit is the one category this sweep adds: overhang.  A used lane
// adds one to its bin in the wavefront's LDS tally, flushed once at the end.
enum { GCB_C_OVERHANG = SW_C_GATE, GCB_C_N = SW_C_GATE + 1, GCB_C_WORDS = SW_C_WORDS };   // (GCB_C_WORDS: the object's counter words behind its bins)

#ifdef QM_EMU
QM_DEV void gcb_load_rec(const unsigned char* r, U4& a, u32& w) { a = load_16(r); w = *(const u32*)(r + 24); }
#else
// both loads in flight before either is looked at (see load_32 in qm_wave.h)
QM_DEV void gcb_load_rec(const unsigned char* r, U4& a, u32& w) {
  typedef u32 v4u __attribute__((ext_vector_type(4)));
  v4u x = *(const v4u*)r; u32 b = *(const u32*)(r + 24);
  asm volatile("" : "+v"(x), "+v"(b));
  a.x = x.x; a.y = x.y; a.z = x.z; a.w = x.w; w = b;
}
#endif

// wavefront `wave` of `nWaves` (both wave-uniform); slab: GCB_SLAB words of its own
QM_DEV void gcb_obs_wave(const UnitSrc& S, const GcbIdx& I, const SweepAcc& A, long long wave, long long nWaves, QM_LDS(u32)* slab) {
  slab_zero(slab, GCB_SLAB);
  u64 ctr[GCB_C_N] = {0, 0, 0, 0, 0, 0, 0};
  for (long long base = wave * 64; base < S.n; base += nWaves * 64) {
    LV<long long> o0, o1;
    unit_bounds(S, base, o0, o1);
    LV<int> cat; LV<u32> bin;
    QM_LANES(l) {
      cat[l] = -1; bin[l] = 0;
      if (base + l >= S.n) continue;
      const long long c = o1[l] - o0[l];
      U4 a{0, 0, 0, 0}; u32 w = 0;
      if (c == 1) gcb_load_rec(S.hits + o0[l] * (long long)S.stride, a, w);
      const u32 f = a.w;
      int k = frag_gate(c, f, w, A.maxLen);
      if (k == SW_C_USED) {
        k = GCB_C_OVERHANG;
        if ((long long)a.x < I.nTxp) {
          const int p = (int)a.y, mp = (int)a.z;
          const long long s = (p > 0 ? p : 0) < (mp > 0 ? mp : 0) ? (p > 0 ? p : 0) : (mp > 0 ? mp : 0), e = s + (long long)f;
          const long long o = I.txpOff[a.x], L = I.txpLen[a.x];
          if (e <= L) { k = SW_C_USED; bin[l] = gcb_bin(gcb_rank_at(I, o + e) - gcb_rank_at(I, o + s), f); }
        }
      }
      cat[l] = k;
    }
    tally<GCB_C_N>(cat, ctr);
    QM_LANES(l) if (cat[l] == SW_C_USED) slab_inc(slab + bin[l]);
  }
  slab_flush(slab, GCB_BINS, A.bins);
  const int word[GCB_C_N] = {SW_C_USED, SW_C_UNMAPPED, SW_C_MULTI, SW_C_NOT_PAIRED, SW_C_SAME_STRAND, SW_C_OUT_OF_RANGE, GCB_C_OVERHANG};
  flush_counters(A.ctr, ctr, word);
}

// ---- the expected matrix: H[t][b] = sum over l of counts[l] * #{ starts s in [0, L_t - l] whose window [s, s + l) falls in bin b }.
//
// The work is cut into tiles of GCB_TILE consecutive starts of one transcript; tileOff (the exclusive scan of the tiles per
// transcript) is the tile table, so long and short transcripts balance.  A wavefront takes a run of consecutive tiles: one binary
// search in the table for the first, then it walks on.  Inside a tile lane i owns start base + i and all lanes walk the length l
// upward together.  The character a window gains at step l is text position P + i with P = off + base + l - 1 wave-uniform: the 64
// bits the lanes need are ONE 64-bit window W of the mask stream, shifted along on the scalar unit, and a lane takes its bit
// straight from W used as a lane mask -- no rank lookup and no load per (s, l).  Lanes past the transcript's end gather characters
// of what follows; they are never counted (lim).
//
// The bin is floor(g * NB / l), capped.  The lanes keep x = 2 * NB * g (< 2^16) instead of g, and the table holds, per length, the
// wave-uniform reciprocal M = ceil(2^31 / l) (<= 2^31: fits 32 bits also at l = 1).  Then mulhi32(x, M) = floor(g * NB * M / 2^31),
// and that is floor(g * NB / l) exactly: with e = M * l - 2^31, 0 <= e < l <= 1023, the product overshoots g * NB / l by
// g * NB * e / (l * 2^31) < 2^15 * 2^10 / (l * 2^31) = 1 / (64 l), less than the 1 / l that separates a quotient with remainder
// l - 1 from the next integer.
//
// Per length the wavefront folds its lanes' bins before anything leaves it: it takes the bin of the first lane not yet counted,
// ballots the lanes that share it, and adds counts[l] * popcount to the accumulator of the lane whose index is the bin.  Adjacent
// windows differ by two characters, so a step sees few distinct bins and the loop ends after a few turns.  A length with
// counts[l] == 0 is skipped wave-uniformly (the lanes still gain their character).  The accumulators go out once per run of tiles
// of a transcript: at most GCB_BINS 64-bit integer atomics.
struct GcbExp {
  const u64* mask; const u32* txpOff; const int* txpLen;
  const long long* tileOff;  // [nTxp + 1]
  const u64* tab;            // [2 * (maxLen + 1)]: counts[l], then ceil(2^31 / l)
  u64* H;                    // [nTxp * GCB_BINS]
  long long nTxp, nTiles;
  int maxLen;
};

#ifdef QM_EMU
QM_DEV bool gcb_lane_bit(u64 W, int l) { return (W >> l) & 1; }
QM_DEV u64 gcb_load_uniform_u64(const u64* p) { return *p; }
#else
// the wave-uniform W as a lane mask (v_cndmask with W as its condition)
QM_DEV bool gcb_lane_bit(u64 W, int) { return __builtin_amdgcn_inverse_ballot_w64(W); }
QM_DEV u64 gcb_load_uniform_u64(const u64* p) { return (u64)load_uniform_i64((const long long*)p); }
#endif

QM_DEV void gcb_tiles_wave(const int* txpLen, long long nTxp, u32* cnt, long long wave) {
  QM_LANES(l) {
    const long long t = wave * 64 + l;
    if (t <= nTxp) cnt[t] = t < nTxp && txpLen[t] > 0 ? (u32)(((long long)txpLen[t] + GCB_TILE - 1) / GCB_TILE) : 0u;
  }
}

QM_DEV void gcb_expect_flush(const GcbExp& E, long long t, LV<u64>& acc) {
  QM_LANES(l) { if (l < GCB_BINS && acc[l]) atomic_add_u64(&E.H[t * GCB_BINS + l], acc[l]); acc[l] = 0; }
}

// wavefront `wave` of `nWaves` (both wave-uniform)
QM_DEV void gcb_expect_wave(const GcbExp& E, long long wave, long long nWaves) {
  const long long per = (E.nTiles + nWaves - 1) / nWaves;
  const long long k0 = wave * per, k1 = k0 + per < E.nTiles ? k0 + per : E.nTiles;
  if (k0 >= k1) return;
  long long lo = 0, hi = E.nTxp;                                 // tileOff[lo] <= k0 < tileOff[hi]
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if (load_uniform_i64(E.tileOff + mid) <= k0) lo = mid; else hi = mid;
  }
  long long t = lo, tEnd = load_uniform_i64(E.tileOff + t + 1);
  LV<u64> acc;
  QM_LANES(l) acc[l] = 0;
  for (long long k = k0; k < k1; ++k) {
    if (k >= tEnd) {
      gcb_expect_flush(E, t, acc);
      do { ++t; tEnd = load_uniform_i64(E.tileOff + t + 1); } while (k >= tEnd);
    }
    const long long base = (k - load_uniform_i64(E.tileOff + t)) * GCB_TILE;
    const long long L = uniform(E.txpLen[t]), P0 = (long long)uniform(E.txpOff[t]) + base;
    const int lmax = (int)(L - base < (long long)E.maxLen ? L - base : (long long)E.maxLen);   // lane 0's last length
    LV<int> lim; LV<u32> x;
    QM_LANES(l) { lim[l] = (int)(L - base) - l; x[l] = 0; }      // lane l counts lengths 1 .. lim[l]
    long long blk = P0 >> 6; int sh = (int)(P0 & 63);
    u64 w0 = gcb_load_uniform_u64(E.mask + blk), w1 = gcb_load_uniform_u64(E.mask + blk + 1);
    for (int len = 1; len <= lmax; ++len) {
      const u64 W = sh ? (w0 >> sh) | (w1 << (64 - sh)) : w0;
      QM_LANES(l) x[l] += gcb_lane_bit(W, l) ? 2u * GCB_BINS : 0u;
      if (++sh == 64) { sh = 0; ++blk; w0 = w1; w1 = gcb_load_uniform_u64(E.mask + blk + 1); }
      const u64 c = gcb_load_uniform_u64(E.tab + 2 * len);
      if (!c) continue;
      const u32 M = (u32)gcb_load_uniform_u64(E.tab + 2 * len + 1);
      LV<u32> bin; LV<bool> act;
      QM_LANES(l) {
        const u32 q = (u32)(((u64)x[l] * M) >> 32);
        bin[l] = q < GCB_BINS - 1 ? q : GCB_BINS - 1; act[l] = len <= lim[l];
      }
      u64 rem = ballot(act);
      while (rem) {
        const u32 b0 = read_lane(bin, ctz64(rem));
        LV<bool> eq;
        QM_LANES(l) eq[l] = act[l] && bin[l] == b0;
        const u64 m = ballot(eq);
        const u64 v = c * (u64)popc64(m);
        QM_LANES(l) if (l == (int)b0) acc[l] += v;
        rem &= ~m;
      }
    }
  }
  gcb_expect_flush(E, t, acc);
}

}  // namespace qm
