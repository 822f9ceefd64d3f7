// qm_psb.inl -- positional bias: where along its transcript a fragment starts and where it ends.  The observed counts (the two bins
// of the fragments of a mapped batch), the expected counts (the same bins over every place a fragment could start or end, weighted:
// a closed form per transcript and bin) and the effective lengths under a table of ratios.  The model is in include/qmap_mi355.h.
//
// Written against qm_wave.h: the same source runs lane by lane under -DQM_EMU (tests/emu/qm_emu_psb.cpp).  Every function here is the
// body of ONE wavefront.  The counts are integer adds and integer atomics only: the same bits whatever the grid.  The effective
// lengths are the walk of qm_sqb.inl (sqb_walk_wave) over another source of end biases: the same order of every float sum.
//
//   psb_class, psb_bin   the class of a transcript length, the bin of a position
//   psb_probe_wave       qm_psb_position: one lane per question
//   psb_obs_wave         the observed sweep, on the frame of qm_sweep.h
//   psb_expect_wave      the expected counts: one lane per (transcript, bin)
//   psb_efflen_wave      sqb_walk_wave over psb_bias: a table lookup by position, no text load
#pragma once
#include <stddef.h>
#include "qm_sqb.inl"

namespace qm {

#define PSB_CLASSES QM_PSB_CLASSES
#define PSB_POS QM_PSB_POS
#define PSB_BINS QM_PSB_BINS
// the observed sweep: a slab of PSB_BINS 32-bit words per wavefront, 800 bytes, 3 200 per workgroup: the compute unit's 32 wavefronts
#define PSB_OBS_BLOCKS_PER_CU 8
// the expected counts: PSB_BINS 64-bit accumulators per wavefront, 1 600 bytes, 6 400 per workgroup
#define PSB_ACC_WORDS (2 * PSB_BINS)
#define PSB_EXP_BLOCKS_PER_CU 8

static_assert(PSB_BINS == 2 * PSB_CLASSES * PSB_POS && PSB_CLASSES == 5 && PSB_POS == 20, "the table's shape");
static_assert(4 * 4 * PSB_ACC_WORDS * PSB_EXP_BLOCKS_PER_CU <= 160 * 1024, "the slabs fit the compute unit's LDS");

struct PsbIdx {              // the transcripts, as they lie in the replica (no text: a position is all this model asks of one)
  const int* txpLen;         // [nTxp]
  long long nTxp;
};

// the class of a transcript of L characters
QM_DEV int psb_class(long long L) { return L <= 791 ? 0 : L <= 1265 ? 1 : L <= 1707 ? 2 : L <= 2433 ? 3 : 4; }

// floor(20 x / L) for 0 <= x < L < 2^31, exact.  20 x needs up to 36 bits: it is kept in 64, and the quotient is first guessed by
// one float64 division -- n = 20 x and L are integers below 2^53, hence exact as doubles, and the true quotient lies in [0, 20), so
// whatever the division's last bits are, the guess is off by less than 1 and its floor by at most one bin -- and then SETTLED by
// integers: the bin is the b with b L <= n < (b + 1) L, and the two comparisons move the guess up or down by one where it does not
// hold.  (A correctly rounded quotient never needs them: the true one lies at least 1 / L below the next integer, 1 / (20 L) > 2^-36
// relative, far more than 2^-53.  The proof does not lean on that.)
QM_DEV int psb_bin(long long x, long long L) {
  const long long n = (long long)PSB_POS * x;
  long long b = (long long)((double)n / (double)L);
  if ((b + 1) * L <= n) ++b;
  if (b * L > n) --b;
  return (int)b;
}

// B_b = ceil(b L / 20): bin b of a transcript of L characters holds the positions [B_b, B_(b+1)); B_0 = 0, B_20 = L
QM_DEV long long psb_edge(long long b, long long L) { return (long long)((u64)(b * L + PSB_POS - 1) / (u64)PSB_POS); }

// out[2 i] = the class of transcript tid[i], out[2 i + 1] = the bin of position pos[i] on it; both -1 where tid[i] is no transcript
// or pos[i] no position of it
QM_DEV void psb_probe_wave(const PsbIdx& I, long long nq, const u32* tid, const int* pos, int* out, long long wave) {
  QM_LANES(l) {
    const long long i = wave * 64 + l;
    if (i >= nq) continue;
    int c = -1, b = -1;
    const u32 t = tid[i];
    if ((long long)t < I.nTxp) {
      const long long L = I.txpLen[t], x = pos[i];
      if (x >= 0 && x < L) { c = psb_class(L); b = psb_bin(x, L); }
    }
    out[2 * i] = c; out[2 * i + 1] = b;
  }
}

// ---- the observed sweep, on the frame of qm_sweep.h: gcb_obs_wave's shape and record loads (16 bytes at 0 and the dword at byte 24
// of a single-hit record, one sector).  A lane that passes frag_gate gathers txpLen and nothing else: no text is read.  One category
// is this sweep's own, the GC sweep's overhang (counter word SW_C_GATE).  A used lane adds one to two words of the wavefront's slab,
// the bin of its start and the bin of its last position; the slab's non-zero words go out at the end, one 64-bit integer atomic each.
enum { PSB_C_OVERHANG = SW_C_GATE, PSB_C_N = SW_C_GATE + 1 };

// wavefront `wave` of `nWaves` (both wave-uniform); slab: PSB_BINS words of its own
QM_DEV void psb_obs_wave(const UnitSrc& S, const PsbIdx& I, const SweepAcc& A, long long wave, long long nWaves, QM_LDS(u32)* slab) {
  slab_zero(slab, PSB_BINS);
  u64 ctr[PSB_C_N] = {0, 0, 0, 0, 0, 0, 0};
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
        k = PSB_C_OVERHANG;
        if ((long long)a.x < I.nTxp) {
          const int p = (int)a.y, mp = (int)a.z;
          const long long s = (p > 0 ? p : 0) < (mp > 0 ? mp : 0) ? (p > 0 ? p : 0) : (mp > 0 ? mp : 0), e = s + (long long)f;
          const long long L = I.txpLen[a.x];
          if (e <= L) {                                              // (f >= 1: 0 <= s <= e - 1 < L)
            k = SW_C_USED;
            const int row = psb_class(L) * PSB_POS;
            slab_inc(slab + row + psb_bin(s, L)); slab_inc(slab + PSB_CLASSES * PSB_POS + row + psb_bin(e - 1, L));
          }
        }
      }
      cat[l] = k;
    }
    tally<PSB_C_N>(cat, ctr);
  }
  slab_flush(slab, PSB_BINS, A.bins);
  const int word[PSB_C_N] = {SW_C_USED, SW_C_UNMAPPED, SW_C_MULTI, SW_C_NOT_PAIRED, SW_C_SAME_STRAND, SW_C_OUT_OF_RANGE, PSB_C_OVERHANG};
  flush_counters(A.ctr, ctr, word);
}

// ---- the expected counts: ONE LANE PER (transcript, bin), item t * PSB_POS + b, the wavefronts striding over the items.  A lane
// takes L_t and q_t, the two edges of its bin and four values of W: a difference of two table values per end, no pass over
// positions.  W is the host's table up to m; beyond it is linear, W[x] = W[m] + (x - m) P[m].  A lane adds its two products to the
// wavefront's PSB_BINS 64-bit accumulators in LDS (one LDS integer atomic each: the lanes of one instruction share words when their
// transcripts share a class); the non-zero words go out once, at the wavefront's end, one 64-bit integer atomic each.  Integers
// only, every sum below 2^63 by the host's refusal: the same bits whatever the grid.
struct PsbExp {
  PsbIdx I;
  const u64* W;              // [maxLen + 1]: W[0] = 0, W[x] = W[x - 1] + P[x]
  const u64* q;              // [nTxp]
  u64* exp;                  // [PSB_BINS]
  u64 Pm;                    // P[maxLen]
  int maxLen;
};

QM_DEV u64 psb_W(const PsbExp& E, long long x) {
  const long long m = E.maxLen;
  return x <= m ? E.W[x] : E.W[m] + (u64)(x - m) * E.Pm;
}

// wavefront `wave` of `nWaves` (both wave-uniform); slab: PSB_ACC_WORDS words of its own
QM_DEV void psb_expect_wave(const PsbExp& E, long long wave, long long nWaves, QM_LDS(u32)* slab) {
  QM_LDS(u64)* acc = (QM_LDS(u64)*)slab;
  QM_LANES(l) for (int i = l; i < PSB_BINS; i += 64) acc[i] = 0;
  wave_fence();
  const long long n = E.I.nTxp * PSB_POS;
  for (long long base = wave * 64; base < n; base += nWaves * 64) {
    QM_LANES(l) {
      const long long i = base + l;
      if (i >= n) continue;
      const long long t = (long long)((u64)i / (u64)PSB_POS), b = i - t * PSB_POS;
      const u64 qt = E.q[t];
      const long long L = E.I.txpLen[t];
      if (!qt || L <= 0) continue;
      const long long B0 = psb_edge(b, L), B1 = psb_edge(b + 1, L);
      if (B0 == B1) continue;                                        // (an empty bin: a transcript shorter than PSB_POS)
      const int at = psb_class(L) * PSB_POS + (int)b;
      sqb_lds_add(acc + at, qt * (psb_W(E, L - B0) - psb_W(E, L - B1)));
      sqb_lds_add(acc + PSB_CLASSES * PSB_POS + at, qt * (psb_W(E, B1) - psb_W(E, B0)));
    }
  }
  wave_fence();
  QM_LANES(l) for (int i = l; i < PSB_BINS; i += 64) { const u64 v = acc[i]; if (v) atomic_add_u64(&E.exp[i], v); }
}

// ---- the effective lengths: the walk of qm_sqb.inl over this model's end biases, b5_t(s) = R[0][c_t][bin_t(s)] and
// b3_t(i) = R[1][c_t][bin_t(i)].  The class is wave-uniform with L; a position costs one psb_bin and one 8-byte load from a table of
// 1 600 bytes, and it is asked once per ring entry and once per start, never inside the walk over the lengths.
QM_DEV double psb_bias(const double* R /*[PSB_BINS]*/, const unsigned char*, long long, long long L, long long x, int end) {
  return R[(end * PSB_CLASSES + psb_class(L)) * PSB_POS + psb_bin(x, L)];
}
// wavefront `wave` of `nWaves` (both wave-uniform); slab: SQB_RING_WORDS words of its own; E.I.text is not looked at
QM_DEV void psb_efflen_wave(const SqbEff& E, long long wave, long long nWaves, QM_LDS(u32)* slab) {
  sqb_walk_wave<psb_bias>(E, wave, nWaves, slab);
}

}  // namespace qm
