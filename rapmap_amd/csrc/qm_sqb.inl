// qm_sqb.inl -- sequence-specific bias: the nucleotide contexts at the two ends of a fragment.  The observed counts (the 18 words of
// the fragments of a mapped batch), the expected counts (the same words over every place a fragment could start or end, weighted),
// and the effective lengths under a table of ratios.  The model is in include/qmap_mi355.h.
//
// Written against qm_wave.h: the same source runs lane by lane under -DQM_EMU (tests/emu/qm_emu_sqb.cpp).  Every function here is the
// body of ONE wavefront.  The counts are integer adds and integer atomics only: the same bits whatever the grid.  The effective
// lengths are float64 in an order the header fixes -- per start, per tile of 64 starts (wave_sum_f64's tree), per transcript in
// ascending tiles -- with plain stores and no floating-point atomic, so they too are the same bits whatever the grid.
//
//   sqb_words          the nine words of one context, or why there are none
//   sqb_probe_wave     qm_sqb_context: one lane per question
//   sqb_obs_wave       the observed sweep, on the frame of qm_sweep.h
//   sqb_expect_wave    the expected counts: one lane per text position over the tile table of qm_gcb.inl (gcb_tiles_wave)
//   sqb_walk_wave      the hot path: a tile's 64 starts walk the fragment length upward over b3 values kept in LDS; a template over
//                      the source of the end biases (sqb_efflen_wave: the sequence model's; psb_efflen_wave, qm_psb.inl: the positional)
//   sqb_tilesum_wave   a transcript's tiles added in order, and the quotient
#pragma once
#include <stddef.h>
#include "qm_gcb.inl"

namespace qm {

#define SQB_CTX QM_SQB_CTX
#define SQB_BINS QM_SQB_BINS
#define SQB_MAX_LEN GCB_MAX_LEN
// the observed sweep: a slab of SQB_BINS 32-bit words per wavefront, 4 608 bytes, 18 KiB per workgroup; 8 workgroups are 144 of the
// compute unit's 160 KiB (and its 32 wavefronts), a ninth does not fit
#define SQB_OBS_BLOCKS_PER_CU 8
// the expected counts: SQB_BINS 64-bit accumulators per wavefront, 9 216 bytes, 36 KiB per workgroup: 4 workgroups are 144 KiB
#define SQB_ACC_WORDS (2 * SQB_BINS)
// the effective lengths: b3 of a run of positions in a ring of SQB_RING doubles per wavefront, its first 64 entries mirrored behind
// it (a lane's read at ring position u + lane never wraps: u alone wraps, on the scalar unit).  A tile needs the positions
// base .. base + 62 + max_len, at most 1 086: what the ring holds in front of base is free to be overwritten.  9 216 bytes again.
#define SQB_RING 1088
#define SQB_RING_WORDS (2 * (SQB_RING + 64))
#define SQB_BLOCKS_PER_CU 4

static_assert(SQB_BINS == 2 * SQB_CTX * 64 && SQB_CTX == 9 && QM_SQB_UP == 3, "the table's shape");
static_assert(SQB_RING % 64 == 0 && SQB_RING >= 63 + SQB_MAX_LEN && 4 * 4 * SQB_RING_WORDS * SQB_BLOCKS_PER_CU <= 160 * 1024 &&
              4 * 4 * SQB_BINS * SQB_OBS_BLOCKS_PER_CU <= 160 * 1024, "the ring holds a tile's span; the slabs fit the compute unit's LDS");

struct SqbIdx {              // the text and the transcripts, as they lie in the replica
  const unsigned char* text;
  const u32* txpOff; const int* txpLen;  // [nTxp]
  long long nTxp, n;
};

// 0 .. 3 for A C G T in either case, 4 for any other byte
QM_DEV u32 sqb_code(u32 c) { c |= 0x20u; return c == 'a' ? 0u : c == 'c' ? 1u : c == 'g' ? 2u : c == 't' ? 3u : 4u; }

enum { SQB_OK = 0, SQB_OFF = 1, SQB_AMBIGUOUS = 2 };
// the nine words of the context of `end` (0: the 5' context of start x, 1: the 3' context of last position x) on a transcript of L
// characters at text + o; SQB_OFF: the context does not lie on the transcript (w untouched), SQB_AMBIGUOUS: a character is not ACGT
QM_DEV int sqb_words(const unsigned char* text, long long o, long long L, long long x, int end, u32* w) {
  const long long lo = end ? x - 5 : x - 3;                      // the first of the nine characters, in text order
  if (lo < 0 || lo + SQB_CTX > L) return SQB_OFF;
  const unsigned char* p = text + o + lo;
  const u64 lo8 = load_u64_unaligned(p); const u32 last = p[8];
  u32 c[SQB_CTX], amb = 0;
#pragma unroll
  for (int j = 0; j < SQB_CTX; ++j) {
    const int k = end ? 8 - j : j;                               // the 3' context reads the other strand: backwards, complemented
    const u32 v = sqb_code(k < 8 ? (u32)(lo8 >> (8 * k)) & 0xffu : last);
    amb |= v >> 2;
    c[j] = (end ? 3u - v : v) & 3u;
  }
  w[0] = c[0]; w[1] = 4 * c[0] + c[1];
#pragma unroll
  for (int j = 2; j < SQB_CTX; ++j) w[j] = 16 * c[j - 2] + 4 * c[j - 1] + c[j];
  return amb ? SQB_AMBIGUOUS : SQB_OK;
}

// out[9 i .. 9 i + 8] = the words of question i, all -1 where its context is not valid
QM_DEV void sqb_probe_wave(const SqbIdx& I, long long nq, const u32* tid, const int* pos, const int* end, int* out, long long wave) {
  QM_LANES(l) {
    const long long i = wave * 64 + l;
    if (i >= nq) continue;
    u32 w[SQB_CTX]; bool ok = false;
    const u32 t = tid[i];
    if ((long long)t < I.nTxp && (end[i] == 0 || end[i] == 1)) ok = sqb_words(I.text, I.txpOff[t], I.txpLen[t], pos[i], end[i], w) == SQB_OK;
    for (int j = 0; j < SQB_CTX; ++j) out[i * SQB_CTX + j] = ok ? (int)w[j] : -1;
  }
}

// ---- the observed sweep, on the frame of qm_sweep.h: gcb_obs_wave's shape and record loads (16 bytes at 0 and the dword at byte 24
// of a single-hit record, one sector).  A lane that passes frag_gate gathers txpOff and txpLen and, where the fragment lies on the
// transcript, its two contexts from the text: nine bytes each, an 8-byte and a 1-byte load.  Two categories are this sweep's own:
// overhang (counter word 6) and ambiguous (word 7, the last free word of SW_C_WORDS).  A used lane adds one to its 18 words in the
// wavefront's slab; the slab's non-zero words go out at the end, one 64-bit integer atomic each (slab_flush).
enum { SQB_C_OVERHANG = SW_C_GATE, SQB_C_AMBIGUOUS = SW_C_GATE + 1, SQB_C_N = SW_C_GATE + 2 };
static_assert((int)SQB_C_N == (int)SW_C_WORDS, "the eight categories fill the frame's counter words");

// wavefront `wave` of `nWaves` (both wave-uniform); slab: SQB_BINS words of its own
QM_DEV void sqb_obs_wave(const UnitSrc& S, const SqbIdx& I, const SweepAcc& A, long long wave, long long nWaves, QM_LDS(u32)* slab) {
  slab_zero(slab, SQB_BINS);
  u64 ctr[SQB_C_N] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (long long base = wave * 64; base < S.n; base += nWaves * 64) {
    LV<long long> o0, o1;
    unit_bounds(S, base, o0, o1);
    LV<int> cat;
    QM_LANES(l) {
      cat[l] = -1;
      if (base + l >= S.n) continue;
      const long long c = o1[l] - o0[l];
      U4 a{0, 0, 0, 0}; u32 w = 0;
      if (c == 1) gcb_load_rec(S.hits + o0[l] * (long long)S.stride, a, w);
      const u32 f = a.w;
      int k = frag_gate(c, f, w, A.maxLen);
      if (k == SW_C_USED) {
        k = SQB_C_OVERHANG;
        if ((long long)a.x < I.nTxp) {
          const int p = (int)a.y, mp = (int)a.z;
          const long long s = (p > 0 ? p : 0) < (mp > 0 ? mp : 0) ? (p > 0 ? p : 0) : (mp > 0 ? mp : 0), e = s + (long long)f;
          const long long o = I.txpOff[a.x], L = I.txpLen[a.x];
          if (e <= L) {
            u32 w5[SQB_CTX], w3[SQB_CTX];
            const int r5 = sqb_words(I.text, o, L, s, 0, w5), r3 = sqb_words(I.text, o, L, e - 1, 1, w3);
            if (r5 != SQB_OFF && r3 != SQB_OFF) {
              k = (r5 | r3) ? SQB_C_AMBIGUOUS : SW_C_USED;
              if (k == SW_C_USED) {
#pragma unroll
                for (int j = 0; j < SQB_CTX; ++j) { slab_inc(slab + j * 64 + w5[j]); slab_inc(slab + (SQB_CTX + j) * 64 + w3[j]); }
              }
            }
          }
        }
      }
      cat[l] = k;
    }
    tally<SQB_C_N>(cat, ctr);
  }
  slab_flush(slab, SQB_BINS, A.bins);
  const int word[SQB_C_N] = {SW_C_USED, SW_C_UNMAPPED, SW_C_MULTI, SW_C_NOT_PAIRED, SW_C_SAME_STRAND, SW_C_OUT_OF_RANGE, SQB_C_OVERHANG, SQB_C_AMBIGUOUS};
  flush_counters(A.ctr, ctr, word);
}

// ---- the expected counts.  The work is cut into gcb_expect_wave's tiles (GCB_TILE consecutive positions of one transcript, the tile
// table from gcb_tiles_wave), a wavefront takes a run of consecutive tiles, lane i owns position x = base + i.
//
// A position serves all nine j of both ends at once: it is character j of the 5' context of start s = x + 3 - j, whose word w_j is
// made of the characters x - 2, x - 1, x whatever j is -- the trimer T5 (its low four bits for j = 1, its low two for j = 0) -- and
// it is character j of the 3' context of last position i = x - 3 + j, whose word is made of the complements of x + 2, x + 1, x: T3.
// The weights are nine consecutive entries of P per end: P[min(m, L - x - 3 + j)] and P[min(m, x - 2 + j)].
//
// Whether a context is valid asks for its nine characters: two ballots per tile give the wavefront one bit per position from
// base - 8 to base + 119 (set: off the transcript or not ACGT), and a lane shifts its 17 bits x - 8 .. x + 8 out of them; the
// context of (end 0, j) covers bits 8 - j .. 16 - j, that of (end 1, j) bits j .. j + 8.
//
// The accumulators are SQB_BINS 64-bit words in the wavefront's LDS (9 216 bytes, SQB_BLOCKS_PER_CU); a lane adds q_t * P[.] with
// one LDS integer atomic per (end, j); the non-zero words go out once, at the wavefront's end, one 64-bit integer atomic each.
struct SqbExp {
  SqbIdx I;
  const long long* tileOff;  // [nTxp + 1]
  const u64* P;              // [maxLen + 1]: fragments of length <= d
  const u64* q;              // [nTxp]
  u64* exp;                  // [SQB_BINS]
  long long nTiles;
  int maxLen;
};

#ifdef QM_EMU
QM_DEV void sqb_lds_add(QM_LDS(u64)* p, u64 v) { *p += v; }
#else
// ds_add_u64 without a return value; the accumulators are this wavefront's own, the lanes of one instruction may share one
QM_DEV void sqb_lds_add(QM_LDS(u64)* p, u64 v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
#endif

// the tile range [k0, k1) of wavefront `wave` and the transcript of tile k0; false: no tile
QM_DEV bool sqb_tile_run(const long long* tileOff, long long nTxp, long long nTiles, long long wave, long long nWaves, long long& k0, long long& k1, long long& t) {
  const long long per = (nTiles + nWaves - 1) / nWaves;
  k0 = wave * per; k1 = k0 + per < nTiles ? k0 + per : nTiles;
  if (k0 >= k1) return false;
  long long lo = 0, hi = nTxp;                                   // tileOff[lo] <= k0 < tileOff[hi]
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if (load_uniform_i64(tileOff + mid) <= k0) lo = mid; else hi = mid;
  }
  t = lo;
  return true;
}

// wavefront `wave` of `nWaves` (both wave-uniform); slab: SQB_ACC_WORDS words of its own
QM_DEV void sqb_expect_wave(const SqbExp& E, long long wave, long long nWaves, QM_LDS(u32)* slab) {
  long long k0, k1, t;
  if (!sqb_tile_run(E.tileOff, E.I.nTxp, E.nTiles, wave, nWaves, k0, k1, t)) return;
  QM_LDS(u64)* acc = (QM_LDS(u64)*)slab;
  QM_LANES(l) for (int i = l; i < SQB_BINS; i += 64) acc[i] = 0;
  wave_fence();
  long long tEnd = load_uniform_i64(E.tileOff + t + 1);
  const long long m = E.maxLen;
  for (long long k = k0; k < k1; ++k) {
    while (k >= tEnd) { ++t; tEnd = load_uniform_i64(E.tileOff + t + 1); }
    const u64 qt = gcb_load_uniform_u64(E.q + t);
    if (!qt) continue;
    const long long base = (k - load_uniform_i64(E.tileOff + t)) * GCB_TILE;
    const long long L = uniform(E.I.txpLen[t]);
    const unsigned char* tx = E.I.text + (long long)uniform(E.I.txpOff[t]);
    LV<bool> b0, b1;
    QM_LANES(l) {
      const long long y0 = base - 8 + l, y1 = base + 56 + l;
      b0[l] = y0 < 0 || y0 >= L || sqb_code(tx[y0]) > 3u;
      b1[l] = y1 >= L || sqb_code(tx[y1]) > 3u;
    }
    const u64 B0 = ballot(b0), B1 = ballot(b1);
    QM_LANES(l) {
      const long long x = base + l;
      if (x >= L) continue;
      const u32 bad = (u32)(l ? (B0 >> l) | (B1 << (64 - l)) : B0) & 0x1ffffu;   // bit n: position x - 8 + n
      // (a character next to x that is off the transcript belongs to no context that lies on it)
      const u32 cm2 = x >= 2 ? sqb_code(tx[x - 2]) : 0u, cm1 = x >= 1 ? sqb_code(tx[x - 1]) : 0u, c0 = sqb_code(tx[x]);
      const u32 cp1 = x + 1 < L ? sqb_code(tx[x + 1]) : 0u, cp2 = x + 2 < L ? sqb_code(tx[x + 2]) : 0u;
      const u32 T5 = (16 * cm2 + 4 * cm1 + c0) & 63u, T3 = (16 * (3u - cp2) + 4 * (3u - cp1) + (3u - c0)) & 63u;
#pragma unroll
      for (int j = 0; j < SQB_CTX; ++j) {
        const u32 keep = j >= 2 ? 63u : j == 1 ? 15u : 3u;
        const long long s = x + 3 - j, i = x - 3 + j;
        if (s >= 3 && s <= L - 6 && !((bad >> (8 - j)) & 0x1ffu)) {
          const long long d = L - s;
          sqb_lds_add(acc + j * 64 + (T5 & keep), qt * E.P[d < m ? d : m]);
        }
        if (i >= 5 && i <= L - 4 && !((bad >> j) & 0x1ffu)) {
          const long long d = i + 1;
          sqb_lds_add(acc + (SQB_CTX + j) * 64 + (T3 & keep), qt * E.P[d < m ? d : m]);
        }
      }
    }
  }
  wave_fence();
  QM_LANES(l) for (int i = l; i < SQB_BINS; i += 64) { const u64 v = acc[i]; if (v) atomic_add_u64(&E.exp[i], v); }
}

// ---- the effective lengths.  Tiles and runs as above; lane i owns start s = base + i and all lanes walk the length l upward
// together.  b3 of the positions a run of tiles needs lies in the wavefront's ring (position p at p % SQB_RING, and again at
// SQB_RING + p when p % SQB_RING < 64): moving on to the next tile of the same transcript computes the 64 positions that tile adds,
// not the 64 + max_len it needs.  At step l lane i reads position s + l - 1: ring entry u + i with u = (base + l - 1) % SQB_RING
// wave-uniform -- one 8-byte LDS read per lane at consecutive addresses (no bank is asked twice within 32 lanes), a product with
// the wave-uniform (double)counts[l], an addition kept where l <= lim.  The lengths with counts come as a list the host makes
// (ascending; upTo[l]: how many of them are <= l), so a length with counts[l] == 0 costs nothing and there is no branch inside
// the walk: four entries are taken at a time -- their eight words in scalar loads, four LDS reads in flight, then the four
// product-and-add pairs in the list's order.  A lane past its lim reads entries that may hold anything; it keeps nothing of them.
struct SqbEff {
  SqbIdx I;
  const long long* tileOff;  // [nTxp + 1]
  const u64* list;           // [2 * upTo[maxLen]]: per length with counts, ascending: the bits of (double)counts[l], then l
  const int* upTo;           // [maxLen + 1]: the list's entries with a length <= l
  const double* R;           // [SQB_BINS]
  double* partial;           // [nTiles]
  long long nTiles;
  int maxLen;
};

// a * b + c with both roundings (never contracted into a fused multiply-add)
QM_DEV double sqb_mul_add(double a, double b, double c) {
#ifndef QM_EMU
#pragma clang fp contract(off)
#endif
  const double p = a * b;
  return p + c;
}
QM_DEV double sqb_bits_f64(u64 b) { double d; __builtin_memcpy(&d, &b, 8); return d; }
// the ring entry of lane 0 at length len, u0 = base % SQB_RING (u0 + len - 1 < 2 * SQB_RING)
QM_DEV int sqb_ring_at(int u0, int len) { const int u = u0 + len - 1; return u >= SQB_RING ? u - SQB_RING : u; }
// ((1.0 * R[end][0][w_0]) * R[end][1][w_1]) ... for a valid context, 1.0 otherwise
QM_DEV double sqb_bias(const double* R, const unsigned char* text, long long o, long long L, long long x, int end) {
  u32 w[SQB_CTX];
  if (sqb_words(text, o, L, x, end, w) != SQB_OK) return 1.0;
  double b = 1.0;
#pragma unroll
  for (int j = 0; j < SQB_CTX; ++j) b = b * R[(end * SQB_CTX + j) * 64 + (int)w[j]];
  return b;
}

// The walk is written once, over the source of the end biases: Bias(E.R, E.I.text, o, L, x, end) is b5 (end 0) of start x or b3
// (end 1) of last position x on the transcript of L characters at text + o (o, L wave-uniform, 0 <= x < L).  It is asked in exactly
// two places: the ring's fill and a tile's 64 starts.  The sequence model's source is sqb_bias, which reads the text; the positional
// model's is a table lookup by position (psb_bias, qm_psb.inl) and leaves the text alone; a joint model is one more function of this
// signature.  (The source is the function itself, called where sqb_bias was called: behind a functor, and behind a type with a
// static member, the sequence instantiation took 47 VGPRs where it had taken 37 -- profiles/psb/results/resources.txt.)
// wavefront `wave` of `nWaves` (both wave-uniform); slab: SQB_RING_WORDS words of its own
template <auto Bias>
QM_DEV void sqb_walk_wave(const SqbEff& E, long long wave, long long nWaves, QM_LDS(u32)* slab) {
  long long k0, k1, t;
  if (!sqb_tile_run(E.tileOff, E.I.nTxp, E.nTiles, wave, nWaves, k0, k1, t)) return;
  QM_LDS(double)* ring = (QM_LDS(double)*)slab;
  long long tEnd = load_uniform_i64(E.tileOff + t + 1);
  long long have = -1;                                           // the ring holds b3 of transcript t up to here (-1: of nothing)
  for (long long k = k0; k < k1; ++k) {
    if (k >= tEnd) {
      do { ++t; tEnd = load_uniform_i64(E.tileOff + t + 1); } while (k >= tEnd);
      have = -1;
    }
    const long long base = (k - load_uniform_i64(E.tileOff + t)) * GCB_TILE;
    const long long L = uniform(E.I.txpLen[t]), o = (long long)uniform(E.I.txpOff[t]);
    const int lmax = (int)(L - base < (long long)E.maxLen ? L - base : (long long)E.maxLen);   // lane 0's last length
    const long long need = base + 63 + lmax < L ? base + 63 + lmax : L;                         // positions [base, need)
    wave_fence();                                                // (the tile before has read what is overwritten now)
    for (long long p0 = have > base ? have : base; p0 < need; p0 += 64) {
      QM_LANES(l) {
        const long long p = p0 + l;
        if (p < need) {
          const double b = Bias(E.R, E.I.text, o, L, p, 1);
          const int ph = (int)(p % SQB_RING);
          ring[ph] = b;
          if (ph < 64) ring[SQB_RING + ph] = b;
        }
      }
    }
    have = need;
    wave_fence();
    LV<int> lim; LV<double> a;
    QM_LANES(l) { lim[l] = (int)(L - base) - l; a[l] = 0.0; }    // lane l counts lengths 1 .. min(lim[l], max_len)
    const int u0 = (int)(base % SQB_RING), ne = uniform(E.upTo[lmax]);
    int e = 0;
    for (; e + 4 <= ne; e += 4) {
      double c[4]; int len[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { c[i] = sqb_bits_f64(gcb_load_uniform_u64(E.list + 2 * (e + i))); len[i] = (int)gcb_load_uniform_u64(E.list + 2 * (e + i) + 1); }
      QM_LANES(l) {
        double b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = ring[sqb_ring_at(u0, len[i]) + l];
#pragma unroll
        for (int i = 0; i < 4; ++i) { const double s = sqb_mul_add(c[i], b[i], a[l]); if (len[i] <= lim[l]) a[l] = s; }
      }
    }
    for (; e < ne; ++e) {
      const double c = sqb_bits_f64(gcb_load_uniform_u64(E.list + 2 * e)); const int len = (int)gcb_load_uniform_u64(E.list + 2 * e + 1);
      QM_LANES(l) { const double s = sqb_mul_add(c, ring[sqb_ring_at(u0, len) + l], a[l]); if (len <= lim[l]) a[l] = s; }
    }
    LV<double> v;
    QM_LANES(l) { const long long x = base + l; v[l] = x < L ? Bias(E.R, E.I.text, o, L, x, 0) * a[l] : 0.0; }
    const double sum = wave_sum_f64(v);
    QM_LANES(l) if (l == 0) E.partial[k] = sum;
  }
}

// the sequence model's instantiation of the walk
QM_DEV void sqb_efflen_wave(const SqbEff& E, long long wave, long long nWaves, QM_LDS(u32)* slab) {
  sqb_walk_wave<sqb_bias>(E, wave, nWaves, slab);
}

// eff[t] = (partial[tileOff[t]] + ... in ascending order) / (double)P[min(L_t, max_len)], or (double)L_t where that P is 0: a lane per transcript
QM_DEV void sqb_tilesum_wave(const int* txpLen, const long long* tileOff, const double* partial, const u64* P, int maxLen, long long nTxp, double* eff, long long wave) {
  QM_LANES(l) {
    const long long t = wave * 64 + l;
    if (t >= nTxp) continue;
    const long long L = txpLen[t] > 0 ? txpLen[t] : 0;
    double s = 0.0;
    for (long long k = tileOff[t]; k < tileOff[t + 1]; ++k) s = s + partial[k];
    const u64 M = P[L < (long long)maxLen ? L : (long long)maxLen];
    eff[t] = M ? s / (double)M : (double)L;
  }
}

}  // namespace qm
