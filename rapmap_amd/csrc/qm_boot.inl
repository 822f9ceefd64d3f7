// qm_boot.inl -- bootstrap replicates of the abundance estimate on the device: resampled class counts and the EM of qm_quant.inl
// over B replicates at once.
//
// The draw.  n_c: the snapshot's counts in snapshot order (ascending slot index), N their sum, cum their exclusive prefix sum.
// Draw j (0 <= j < N) of replicate number R under `seed`:
//   k = j >> 1;  (x0, x1, x2, x3) = Philox4x32-10(counter = (lo k, hi k, lo R, hi R), key = (lo seed, hi seed))
//   u = (j & 1) ? (x2 | x3 << 32) : (x0 | x1 << 32);  p = mulhi64(u, N);  the class is the c with cum[c] <= p < cum[c + 1]
// One lane per Philox call (two draws); the counts are integer atomic adds, which commute: a replicate's counts depend on
// (snapshot, seed, R) alone.
//
// The EM.  The model is qm_quant.inl's, per replicate, with its single-tid rule and quant_mul_add.  Every per-replicate array is
// replicate-innermost, x[item * Bp + rep] (Bp: the replicates rounded up to BOOT_TILE), so that one gathered item is a run of
// BOOT_TILE contiguous doubles: four whole 32-byte sectors.  A wavefront takes BOOT_ROWS rows x BOOT_TILE replicates: lane l has
// row l / 16 of its four and replicate l % 16 of its tile, and reads the index arrays once for the sixteen replicates.
// Written against qm_wave.h: the same source runs lane by lane under -DQM_EMU (tests/emu/qm_emu_boot.cpp).  Every function here is
// the body of ONE wavefront; qm_boot_host.inl launches them (qm_exec.h).  No floating-point atomic anywhere.
//
//   boot_counts_wave      the snapshot's counts (doubles in the quant object) as 64-bit integers: what cum is scanned from
//   boot_rowflag_wave     per row of a side: more than BOOT_LONG items?  (a scan and quant_queue_wave make the side's queue)
//   boot_resample_wave    64 Philox calls of one replicate: 128 draws, each a binary search over cum and one atomic add
//   boot_single_wave      single[t] of every replicate from the one-tid classes, as quant_compact_wave has it for Quant
//   boot_column_wave      one replicate's counts out of / into the replicate-innermost array (set_counts, fetch_counts)
//   boot_start_wave       start values and weights of a range of replicates; boot_reset_wave: their bookkeeping
//   boot_class_wave       r from w;  boot_txp_wave: alpha and the next w from r, and on a checking iteration every replicate's
//                         largest relative change into ITS OWN word (an integer atomic max over the bits)
//                         (boot_start_vb_wave, boot_txp_vb_wave: the same bodies with the variational weight of qm_quant.inl)
//   boot_mark_wave        after a checking iteration: replicates whose word is below rel_tol are done (frozen from here on)
//   boot_begin_wave / boot_end_wave   a run's per-replicate iteration counts
//   boot_transpose_wave   alpha[t * Bp + rep] -> out[rep * nTxps + t]
#pragma once
#include "qm_quant.inl"

namespace qm {

#define BOOT_TILE 16          // replicates per wavefront: 128 bytes per gathered item
#define BOOT_ROWS 4           // rows per wavefront
#define BOOT_LONG 32          // a row of more than this many items is walked by a wavefront of its own (per tile)
enum { BOOT_SC_DONE = 0,      // replicates that are done (the one word the host reads on a checking iteration)
       BOOT_SC_WORDS = 8 };

struct BootState {
  QuantCsr cls, txp;          // the quant object's graph; queue: the rows of more than BOOT_LONG items
  const double* eff;          // [transcripts]
  const u64* cnt;             // [classes][Bp]
  const double* single;       // [transcripts][Bp]
  double* w; double* r; double* alpha;          // [transcripts][Bp], [classes][Bp], [transcripts][Bp]: alpha is updated in place
  u64* rel;                   // [Bp]: bits of the largest relative change of a checking iteration
  const u32* done;            // [Bp]: 1 = frozen (the padding beyond the replicates is done from the start)
  long long Bp; double minAlpha; int check;
};

constexpr long long boot_row_waves(long long n) { return (n + BOOT_ROWS - 1) / BOOT_ROWS; }
constexpr long long boot_side_waves(const QuantCsr& A) { return boot_row_waves(A.n) + A.nq; }
constexpr long long boot_padded(long long nReps) { return (nReps + BOOT_TILE - 1) / BOOT_TILE * BOOT_TILE; }

// ---- Philox4x32-10 (Salmon, Thomas, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), from its description:
// a round takes (c0, c1, c2, c3) to (hi(M1 * c2) ^ c1 ^ k0, lo(M1 * c2), hi(M0 * c0) ^ c3 ^ k1, lo(M0 * c0)); ten rounds, the
// key bumped by the Weyl constants after each.
QM_DEV void boot_philox(u32 c0, u32 c1, u32 c2, u32 c3, u32 k0, u32 k1, u32* out) {
  for (int round = 0; round < 10; ++round) {
    const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
    const u32 n0 = (u32)(p1 >> 32) ^ c1 ^ k0, n2 = (u32)(p0 >> 32) ^ c3 ^ k1;
    c1 = (u32)p1; c3 = (u32)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// the class of position p: the c in [0, nc) with cum[c] <= p < cum[c + 1] (cum[0] = 0, cum[nc] = N > p)
QM_DEV long long boot_find_class(const u64* cum, long long nc, u64 p) {
  long long lo = 0, hi = nc;
  while (hi - lo > 1) { const long long mid = (lo + hi) >> 1; if (cum[mid] <= p) lo = mid; else hi = mid; }
  return lo;
}

struct BootDraw {
  const u64* cum; long long nc; u64 N; u64 seed; u64 firstRep;
  u64* cnt; long long Bp; int aggregate;      // aggregate: equal classes within a wavefront meet before one lane issues the atomic
};

// wavefront `wave` of replicate slot `slot`: Philox calls wave * 64 .. + 63, two draws each (the last call of an odd N: one)
QM_DEV void boot_resample_wave(const BootDraw& D, long long wave, long long slot) {
  const u64 R = D.firstRep + (u64)slot;
  LV<long long> cls[2];
  QM_LANES(l) {
    const u64 k = (u64)wave * 64 + (u64)l;
    cls[0][l] = -1; cls[1][l] = -1;
    if (2 * k >= D.N) continue;
    u32 x[4];
    boot_philox((u32)k, (u32)(k >> 32), (u32)R, (u32)(R >> 32), (u32)D.seed, (u32)(D.seed >> 32), x);
    cls[0][l] = boot_find_class(D.cum, D.nc, mulhi64((u64)x[0] | ((u64)x[1] << 32), D.N));
    if (2 * k + 1 < D.N) cls[1][l] = boot_find_class(D.cum, D.nc, mulhi64((u64)x[2] | ((u64)x[3] << 32), D.N));
  }
  if (!D.aggregate) {
    QM_LANES(l) for (int h = 0; h < 2; ++h) if (cls[h][l] >= 0) atomic_add_u64(&D.cnt[cls[h][l] * D.Bp + slot], 1);
    return;
  }
  // the lowest lane that still holds a draw names its class; every lane that holds the same one drops out, the namer adds their number
  for (int h = 0; h < 2; ++h) {
    LV<bool> open; LV<u64> c64;
    QM_LANES(l) { open[l] = cls[h][l] >= 0; c64[l] = (u64)cls[h][l]; }
    for (u64 m = ballot(open); m; m = ballot(open)) {
      const int lead = ctz64(m);
      const u64 target = read_lane(c64, lead);
      LV<bool> same;
      QM_LANES(l) same[l] = open[l] && c64[l] == target;
      const u64 sm = ballot(same);
      QM_LANES(l) { if (l == lead) atomic_add_u64(&D.cnt[(long long)target * D.Bp + slot], (u64)popc64(sm)); if (same[l]) open[l] = false; }
    }
  }
}

// ---- structure and bookkeeping
QM_DEV void boot_counts_wave(const double* dcnt, long long nc, u64* out, long long wave) {
  QM_LANES(l) { const long long c = wave * 64 + l; if (c <= nc) out[c] = c < nc ? (u64)dcnt[c] : 0; }   // (out[nc] = 0: the scan's total lands there)
}
QM_DEV void boot_rowflag_wave(const long long* off, long long n, u32* flag, long long wave) {
  QM_LANES(l) { const long long i = wave * 64 + l; if (i <= n) flag[i] = (i < n && off[i + 1] - off[i] > BOOT_LONG) ? 1u : 0u; }
}
// lane l: class wave * 4 + l / 16, replicate slot tile * 16 + l % 16 (every slot of the padded width: the padding holds zeros)
QM_DEV void boot_single_wave(const long long* coff, const u32* clab, long long nc, const u64* cnt, double* single, long long Bp, long long wave, long long tile) {
  QM_LANES(l) {
    const long long c = wave * BOOT_ROWS + l / BOOT_TILE, b = tile * BOOT_TILE + (l & (BOOT_TILE - 1));
    if (c >= nc || coff[c + 1] - coff[c] != 1) continue;
    single[(long long)clab[coff[c]] * Bp + b] = (double)cnt[c * Bp + b];
  }
}
// put = 1: col[c] into cnt[c][slot], and single[t][slot] of a one-tid class {t}; put = 0: cnt[c][slot] into col[c]
QM_DEV void boot_column_wave(const long long* coff, const u32* clab, long long nc, u64* cnt, double* single, long long Bp, long long slot, u64* col, int put, long long wave) {
  QM_LANES(l) {
    const long long c = wave * 64 + l;
    if (c >= nc) continue;
    if (!put) { col[c] = cnt[c * Bp + slot]; continue; }
    cnt[c * Bp + slot] = col[c];
    if (coff[c + 1] - coff[c] == 1) single[(long long)clab[coff[c]] * Bp + slot] = (double)col[c];
  }
}
// slots s0 .. s0 + ns - 1 start anew: `value` for the transcripts that occur in a label, 0 for all others, and the weights of that
// (VB: quant_weight's method, decided when the kernel is compiled; prior: [transcripts], the same for every replicate)
template <int VB>
QM_DEV void boot_start_body(const long long* toff, const double* eff, const double* prior, long long nTxps, double value, double* alpha, double* w, long long Bp,
                            long long s0, long long ns, long long wave, long long tile) {
  QM_LANES(l) {
    const long long t = wave * BOOT_ROWS + l / BOOT_TILE, b = tile * BOOT_TILE + (l & (BOOT_TILE - 1));
    if (t >= nTxps || b < s0 || b >= s0 + ns) continue;
    const double a = toff[t + 1] > toff[t] ? value : 0.0;
    alpha[t * Bp + b] = a; w[t * Bp + b] = quant_weight<VB>(a, prior, t, eff[t]);
  }
}
QM_DEV void boot_start_wave(const long long* toff, const double* eff, long long nTxps, double value, double* alpha, double* w, long long Bp, long long s0, long long ns,
                            long long wave, long long tile) {
  boot_start_body<0>(toff, eff, nullptr, nTxps, value, alpha, w, Bp, s0, ns, wave, tile);
}
QM_DEV void boot_start_vb_wave(const long long* toff, const double* eff, const double* prior, long long nTxps, double value, double* alpha, double* w, long long Bp,
                               long long s0, long long ns, long long wave, long long tile) {
  boot_start_body<1>(toff, eff, prior, nTxps, value, alpha, w, Bp, s0, ns, wave, tile);
}
struct BootBook {             // per replicate slot, [Bp]
  u32* done; u64* rel; int* iters; double* lastRel; u64* scal;
};
QM_DEV void boot_reset_wave(const BootBook& K, long long s0, long long ns, long long wave) {
  LV<bool> was;
  QM_LANES(l) {
    const long long b = s0 + wave * 64 + l;
    was[l] = false;
    if (b >= s0 + ns) continue;
    was[l] = K.done[b] != 0;
    K.done[b] = 0; K.rel[b] = 0; K.iters[b] = 0; K.lastRel[b] = -1.0;
  }
  const u64 m = ballot(was);
  if (m) { QM_LANES(l) if (l == 0) atomic_add_u64(&K.scal[BOOT_SC_DONE], (u64)0 - (u64)popc64(m)); }
}
// a run begins: no iteration of this call yet; a replicate that is still running has not been looked at in this call
QM_DEV void boot_begin_wave(const BootBook& K, long long nReps, long long wave) {
  QM_LANES(l) { const long long b = wave * 64 + l; if (b < nReps) { K.iters[b] = 0; if (!K.done[b]) K.lastRel[b] = -1.0; } }
}
// after checking iteration `it` of a run: the word of every running replicate is kept as its last relative change and cleared;
// below relTol the replicate is done after `it` iterations of this call
QM_DEV void boot_mark_wave(const BootBook& K, long long nReps, int it, double relTol, long long wave) {
  LV<bool> now;
  QM_LANES(l) {
    const long long b = wave * 64 + l;
    now[l] = false;
    if (b >= nReps || K.done[b]) continue;
    double rel; const u64 bits = K.rel[b]; __builtin_memcpy(&rel, &bits, 8);
    K.lastRel[b] = rel; K.rel[b] = 0;
    if (rel < relTol) { K.done[b] = 1; K.iters[b] = it; now[l] = true; }
  }
  const u64 m = ballot(now);
  if (m) { QM_LANES(l) if (l == 0) atomic_add_u64(&K.scal[BOOT_SC_DONE], (u64)popc64(m)); }
}
// a run ends after `it` iterations: what is still running has made them all
QM_DEV void boot_end_wave(const BootBook& K, long long nReps, int it, long long wave) {
  QM_LANES(l) { const long long b = wave * 64 + l; if (b < nReps && !K.done[b]) K.iters[b] = it; }
}
QM_DEV void boot_transpose_wave(const double* alpha, long long nTxps, long long Bp, double* out, long long wave, long long slot) {
  QM_LANES(l) { const long long t = wave * 64 + l; if (t < nTxps) out[slot * nTxps + t] = alpha[t * Bp + slot]; }
}

// ---- iteration.  Wavefront `wave` of a launch over side A, replicate tile `tile`: live[l] says whether lane l's replicate is still
// running (a wavefront none of whose sixteen is returns false at once: nothing of a done replicate is read or written), row[l] >= 0
// in the lanes that finish a row for their replicate, sum[l] there the sum of x[item][replicate] over the row's items.
// Order of the additions, the same for every replicate, tile and slot: a row of up to BOOT_LONG items: ((x0 + x1) + x2) + ...,
// the items as they lie; a longer row (one wavefront per row and tile): quarter g = 0 .. 3 adds items g, g + 4, g + 8, ... in that
// order from 0.0, then the quarters meet as (q0 + q1) + (q2 + q3).
QM_DEV bool boot_row_sums(const BootState& S, const QuantCsr& A, const double* x, long long wave, long long tile, LV<bool>& live, LV<long long>& row, LV<double>& sum) {
  QM_LANES(l) { live[l] = !S.done[tile * BOOT_TILE + (l & (BOOT_TILE - 1))]; row[l] = -1; sum[l] = 0.0; }
  if (!ballot(live)) return false;
  const long long rw = boot_row_waves(A.n);
  if (wave < rw) {
    QM_LANES(l) {
      const long long i = wave * BOOT_ROWS + l / BOOT_TILE, b = tile * BOOT_TILE + (l & (BOOT_TILE - 1));
      if (i >= A.n || !live[l]) continue;
      const long long o = A.off[i], c = A.off[i + 1] - o;
      if (c > BOOT_LONG) continue;                                 // the queue part's
      double a = 0.0;
      for (long long k = 0; k < c; ++k) a += x[(long long)A.idx[o + k] * S.Bp + b];
      sum[l] = a; row[l] = i;
    }
  } else {
    const long long i = A.queue[wave - rw];
    const long long o = A.off[i], c = A.off[i + 1] - o;
    QM_LANES(l) {
      const long long b = tile * BOOT_TILE + (l & (BOOT_TILE - 1));
      double a = 0.0;
      if (live[l]) for (long long k = l / BOOT_TILE; k < c; k += BOOT_ROWS) a += x[(long long)A.idx[o + k] * S.Bp + b];
      sum[l] = a;
    }
    quarters_sum_f64(sum);
    QM_LANES(l) if (l < BOOT_TILE && live[l]) row[l] = i;
  }
  return true;
}

QM_DEV void boot_class_wave(const BootState& S, long long wave, long long tile) {
  LV<bool> live; LV<long long> row; LV<double> d;
  if (!boot_row_sums(S, S.cls, S.w, wave, tile, live, row, d)) return;
  QM_LANES(l) {
    const long long c = row[l], b = tile * BOOT_TILE + (l & (BOOT_TILE - 1));
    if (c < 0) continue;
    const bool one = S.cls.off[c + 1] - S.cls.off[c] == 1;       // a single-tid class: its count goes to its transcript as it is (S.single)
    S.r[c * S.Bp + b] = (one || d[l] < QNT_DBL_MIN) ? 0.0 : (double)S.cnt[c * S.Bp + b] / d[l];
  }
}

template <int VB>
QM_DEV void boot_txp_body(const BootState& S, const double* prior, long long wave, long long tile) {
  LV<bool> live; LV<long long> row; LV<double> s;
  if (!boot_row_sums(S, S.txp, S.r, wave, tile, live, row, s)) return;
  QM_LANES(l) {
    const long long t = row[l], b = tile * BOOT_TILE + (l & (BOOT_TILE - 1));
    if (t < 0) continue;
    const long long at = t * S.Bp + b;
    const double wt = S.w[at];
    const double a1 = quant_mul_add(wt, s[l], wt < QNT_DBL_MIN ? 0.0 : S.single[at]);
    if (S.check && a1 > S.minAlpha) {
      const double rel = __builtin_fabs(a1 - S.alpha[at]) / a1;
      u64 bits; __builtin_memcpy(&bits, &rel, 8);                // rel >= 0: the bits order as the numbers do
      if (bits > S.rel[b]) atomic_max_u64(&S.rel[b], bits);      // (the word only rises within a launch: a stale read costs an atomic, no more)
    }
    S.alpha[at] = a1; S.w[at] = quant_weight<VB>(a1, prior, t, S.eff[t]);   // (alpha and w of (t, replicate) are this lane's alone in this launch)
  }
}
QM_DEV void boot_txp_wave(const BootState& S, long long wave, long long tile) { boot_txp_body<0>(S, nullptr, wave, tile); }
QM_DEV void boot_txp_vb_wave(const BootState& S, const double* prior, long long wave, long long tile) { boot_txp_body<1>(S, prior, wave, tile); }

}  // namespace qm
