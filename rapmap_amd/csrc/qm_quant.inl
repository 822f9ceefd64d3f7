// qm_quant.inl -- abundance estimation on the device: the EM over the equivalence-class table (qm_eqc.inl).
//
// The model, all in float64 (alpha_t: the fragments assigned to transcript t, e_t its effective length, n_c the count of class c
// and L_c its label):
//   w_t = alpha_t / e_t      d_c = sum of w_t over t in L_c      r_c = n_c / d_c (0 when d_c < DBL_MIN)
//   alpha'_t = w_t * (sum of r_c over the classes c that contain t)
// A class of ONE tid is taken out of the sums: there d_c = w_t and w_t * (n_c / w_t) is n_c, which two roundings do not always give
// back -- its count is kept per transcript (`single`) and added as it is (unless w_t < DBL_MIN: the class is skipped, as above), and
// its r_c is 0.  A transcript that occurs in single-tid classes only then holds exactly its count, whatever the iteration.
// Written against qm_wave.h: the same source runs lane by lane under -DQM_EMU (tests/emu/qm_emu_quant.cpp).  Every function here
// is the body of ONE wavefront; qm_quant_host.inl launches them (qm_exec.h).  No floating-point atomic anywhere: every sum is
// taken by one wavefront, in an order that the structure alone fixes.
//
// Structure build (once per quant object)
//   quant_mark_wave       per slot of the table: published?  how many tids?   (two exclusive scans follow: class index, label offset)
//   quant_compact_wave    per published slot: label, count (as a double) and the (tid, class) pairs of the transpose, in class order;
//                         a tid beyond the transcripts is COUNTED (one word), never acted on
//   (a stable sort of the pairs by tid follows: the transcript side, classes ascending within a transcript)
//   quant_bounds_wave     per transcript: where its run of the sorted pairs begins
//   quant_rowstat_wave    per row of a side (QuantCsr): rows of more than QNT_GROUP items are flagged for the side's queue, the
//                         longest row and the rows that are not empty are folded into the scalar block (integer atomics)
//   quant_queue_wave      the flagged rows into the queue, at the places an exclusive scan of the flags gave them
// Iteration (two launches)
//   quant_class_wave      r_c from w: a launch over the class side
//   quant_txp_wave        alpha'_t and the next w_t from r: a launch over the transcript side; on a checking iteration the largest
//                         relative change is folded into one word (an integer atomic max over the bits of a non-negative double)
//   quant_txp_vb_wave     the same body with the variational weight w_t = E(alpha_t + p_t) / e_t (quant_weight, quant_exp_digamma); the
//                         method is a template parameter of the body: the EM's kernels are what they were
//   Both go through quant_row_sums: the first ceil(rows / 8) wavefronts of a launch take eight rows each, eight lanes per row (rows
//   of up to QNT_GROUP items), the remaining ones one queued row each (a strided loop per lane, then the sum over the wavefront).
#pragma once
#include "qm_eqc.inl"

namespace qm {

enum { QNT_SC_BAD_TID = 0,    // label entries that name a transcript >= nTxps
       QNT_SC_PRESENT = 1,    // transcripts that occur in at least one label
       QNT_SC_MAX_LABEL = 2,  // the longest label
       QNT_SC_MAX_LIST = 3,   // the longest transcript list
       QNT_SC_REL = 4,        // bits of the largest relative change of a checking iteration
       QNT_SC_WORDS = 8 };
#define QNT_GROUP 8           // lanes per row in the group part of a launch
#define QNT_DBL_MIN 2.2250738585072014e-308

struct QuantCsr {             // one side of the bipartite graph: row i's items are idx[off[i] .. off[i + 1])
  const long long* off; const u32* idx; long long n;
  const long long* queue; long long nq;     // the rows of more than QNT_GROUP items
};
struct QuantState {
  QuantCsr cls, txp;          // class -> its tids; transcript -> its classes, ascending
  const double* cnt;          // [classes]
  const double* eff;          // [transcripts]
  const double* single;       // [transcripts]: the count of the class {t}, 0.0 without one
  double* w; double* r;
  const double* alpha; double* alphaNew;
  u64* scal; double minAlpha; int check;
};
struct QuantBuild {           // the structure build's view: the table and what is made of it
  const u64* key; const u32* llen; const long long* loff; const u64* count; const u32* pool; long long cap;
  u32* flag; u32* len;        // [cap + 1]
  const long long* cidx; const long long* lofs;   // [cap + 1]: the scans of flag and len
  long long* coff; u32* clab; double* cnt; u32* pairTid; u32* pairCls;
  double* single;             // [nTxps], zeroed before the compact launch
  u64 nTxps; u64* scal;
};

// (constexpr: the launch wrappers on the host count wavefronts the same way)
constexpr long long quant_group_waves(long long n) { return (n + 64 / QNT_GROUP - 1) / (64 / QNT_GROUP); }

// ---- structure build
QM_DEV void quant_mark_wave(const QuantBuild& B, long long wave) {
  QM_LANES(l) {
    const long long s = wave * 64 + l;
    if (s > B.cap) continue;
    const bool pub = s < B.cap && B.key[s] != 0;
    B.flag[s] = pub ? 1u : 0u; B.len[s] = pub ? B.llen[s] : 0u;
  }
}

QM_DEV void quant_compact_wave(const QuantBuild& B, long long wave) {
  LV<int> bad;
  QM_LANES(l) {
    bad[l] = 0;
    const long long s = wave * 64 + l;
    if (s > B.cap) continue;
    const long long c = B.cidx[s], o = B.lofs[s];
    if (s == B.cap) { B.coff[c] = o; continue; }                // one past the last class: the end of the labels
    if (!B.key[s]) continue;
    const u32 n = B.llen[s]; const u32* L = B.pool + B.loff[s];
    B.coff[c] = o; B.cnt[c] = (double)B.count[s];
    for (u32 j = 0; j < n; ++j) {
      const u32 t = L[j];
      B.clab[o + j] = t; B.pairTid[o + j] = t; B.pairCls[o + j] = (u32)c;
      if ((u64)t >= B.nTxps) bad[l]++;
      else if (n == 1) B.single[t] = (double)B.count[s];        // (labels are distinct: one class {t} at the most)
    }
  }
  lane_scan_add(bad);                                            // counted, one atomic per wavefront: no lane leaves early
  const int nb = read_lane(bad, 63);
  if (nb) { QM_LANES(l) if (l == 0) atomic_add_u64(&B.scal[QNT_SC_BAD_TID], (u64)nb); }
}

// bound[t] = the first position of the sorted tids that holds t or more, t = 0 .. nTxps (bound[nTxps] = n when every tid is below nTxps)
QM_DEV void quant_bounds_wave(const u32* sortedTid, long long n, long long nTxps, long long* bound, long long wave) {
  QM_LANES(l) {
    const long long t = wave * 64 + l;
    if (t > nTxps) continue;
    long long lo = 0, hi = n;
    while (lo < hi) { const long long mid = (lo + hi) >> 1; if ((long long)sortedTid[mid] < t) lo = mid + 1; else hi = mid; }
    bound[t] = lo;
  }
}

// flag[i] = row i has more than QNT_GROUP items (flag[n] = 0: the scan's total); the longest row into scal[maxWord], and with
// `present` the rows that are not empty into scal[QNT_SC_PRESENT]
QM_DEV void quant_rowstat_wave(const long long* off, long long n, u32* flag, u64* scal, int maxWord, int present, long long wave) {
  LV<int> len; LV<bool> some;
  QM_LANES(l) {
    const long long i = wave * 64 + l;
    len[l] = 0; some[l] = false;
    if (i > n) continue;
    if (i < n) { len[l] = (int)(off[i + 1] - off[i]); some[l] = len[l] > 0; }
    flag[i] = len[l] > QNT_GROUP ? 1u : 0u;
  }
  const int mx = wave_max(len);
  const u64 sm = ballot(some);
  QM_LANES(l) if (l == 0) {
    if (mx > 0) atomic_max_u64(&scal[maxWord], (u64)mx);
    if (present && sm) atomic_add_u64(&scal[QNT_SC_PRESENT], (u64)popc64(sm));
  }
}

QM_DEV void quant_queue_wave(const u32* flag, const long long* pos, long long n, long long* queue, long long wave) {
  QM_LANES(l) { const long long i = wave * 64 + l; if (i < n && flag[i]) queue[pos[i]] = i; }
}

// the uniform start: `value` for the transcripts that occur in a label, 0 for all others
QM_DEV void quant_start_wave(const long long* toff, long long nTxps, double value, double* alpha, long long wave) {
  QM_LANES(l) { const long long t = wave * 64 + l; if (t < nTxps) alpha[t] = toff[t + 1] > toff[t] ? value : 0.0; }
}
// ---- the variational method.  E(x) = exp(digamma(x)) for x >= QNT_VB_X_MIN, 0.0 below it, defined by
// the operations below and by nothing else: + - * / on doubles, comparisons, one conversion to an integer and the exponent bits
// of two powers of two, never contracted -- the device, the lane emulation and tests/vb_cases.py give the same 64 bits.
//   y = x, s = 0; while y < 10: s += 1 / y, y += 1                   (digamma(x) = digamma(y) - s; ten steps at the most)
//   digamma(y) = log y + t,  t = -1/(2y) - 1/(12 y^2) + 1/(120 y^4) - 1/(252 y^6) + 1/(240 y^8) - 1/(132 y^10) + 691/(32760 y^12)
//   E(x) = y * exp(t - s): no logarithm is taken.  u = t - s <= 0; below -750 the answer is 0.0 (y * exp(u) is under half the
//   smallest subnormal); k = the integer nearest u / ln 2, r = u - k ln 2 in two pieces (the high one has 32 bits: k times it is
//   exact), exp(r) by its Taylor polynomial of degree 14 (|r| <= 0.35: the remainder is below 1e-19), and 2^k in two halves, so
//   that each is a normal number and the one rounding of a subnormal answer is the last multiplication's.
#define QNT_VB_X_MIN 1e-10
QM_DEV double quant_pow2(long long e) {                            // 2^e, -1022 <= e <= 1023, from its exponent bits
  const u64 bits = (u64)(1023 + e) << 52;
  double p; __builtin_memcpy(&p, &bits, 8);
  return p;
}
QM_DEV double quant_exp_digamma(double x) {
#ifndef QM_EMU
#pragma clang fp contract(off)
#endif
  if (!(x >= QNT_VB_X_MIN)) return 0.0;
  double y = x, s = 0.0;
  while (y < 10.0) { s += 1.0 / y; y += 1.0; }
  const double z = 1.0 / y, z2 = z * z;
  double p = 0.021092796092796094;                                  // 691/32760, then 1/132, 1/240, 1/252, 1/120, 1/12
  p = 0.007575757575757576 - z2 * p;
  p = 0.004166666666666667 - z2 * p;
  p = 0.003968253968253968 - z2 * p;
  p = 0.008333333333333333 - z2 * p;
  p = 0.08333333333333333 - z2 * p;
  const double u = (-0.5 * z - z2 * p) - s;
  if (!(u >= -750.0)) return 0.0;
  const long long k = (long long)(u * 1.4426950408889634 - 0.5);    // (u <= 0: the conversion truncates towards zero)
  const double kf = (double)k;
  const double r = (u - kf * 0.6931471803691238) - kf * 1.9082149292705877e-10;
  double q = 1.1470745597729725e-11;                                // 1/14!, then 1/13! .. 1/2!, 1, 1
  q = 1.6059043836821613e-10 + r * q;
  q = 2.08767569878681e-09 + r * q;
  q = 2.505210838544172e-08 + r * q;
  q = 2.755731922398589e-07 + r * q;
  q = 2.7557319223985893e-06 + r * q;
  q = 2.48015873015873e-05 + r * q;
  q = 0.0001984126984126984 + r * q;
  q = 0.001388888888888889 + r * q;
  q = 0.008333333333333333 + r * q;
  q = 0.041666666666666664 + r * q;
  q = 0.16666666666666666 + r * q;
  q = 0.5 + r * q;
  q = 1.0 + r * q;
  q = 1.0 + r * q;
  const long long h = (-k) >> 1;
  return ((y * q) * quant_pow2(-h)) * quant_pow2(k + h);
}
QM_DEV void quant_exp_digamma_wave(const double* x, long long n, double* out, long long wave) {
  QM_LANES(l) { const long long i = wave * 64 + l; if (i < n) out[i] = quant_exp_digamma(x[i]); }
}

// w_t of a transcript from its current alpha: VB = 0 the EM's alpha / e, VB = 1 the variational E(alpha + prior) / e (the method
// is decided when the kernel is compiled: an EM kernel holds nothing of E and reads no prior)
template <int VB>
QM_DEV double quant_weight(double alpha, const double* prior, long long t, double eff) {
  if (VB) return quant_exp_digamma(alpha + prior[t]) / eff;
  return alpha / eff;
}

QM_DEV void quant_weights_wave(const double* alpha, const double* eff, long long nTxps, double* w, long long wave) {
  QM_LANES(l) { const long long t = wave * 64 + l; if (t < nTxps) w[t] = alpha[t] / eff[t]; }
}
QM_DEV void quant_weights_vb_wave(const double* alpha, const double* eff, const double* prior, long long nTxps, double* w, long long wave) {
  QM_LANES(l) { const long long t = wave * 64 + l; if (t < nTxps) w[t] = quant_weight<1>(alpha[t], prior, t, eff[t]); }
}

// ---- iteration.  Wavefront `wave` of a launch over side A: row[l] >= 0 in the ONE lane that finishes a row (the first lane of
// its group; lane 0 for a queued row), sum[l] there the sum of x over the row's items.  All 64 lanes stay active throughout.
// Order of the additions: a row of up to 8 items: ((x0 + x1) + (x2 + x3)) + ((x4 + x5) + (x6 + x7)), absent items 0.0; a queued row:
// lane l adds items l, l + 64, ... in that order, then the lanes' sums meet as wave_sum_f64 has it.
QM_DEV void quant_row_sums(const QuantCsr& A, const double* x, long long wave, LV<long long>& row, LV<double>& sum) {
  const long long gw = quant_group_waves(A.n);
  if (wave < gw) {
    QM_LANES(l) {
      const long long i = wave * (64 / QNT_GROUP) + l / QNT_GROUP; const int j = l & (QNT_GROUP - 1);
      row[l] = -1; sum[l] = 0.0;
      if (i >= A.n) continue;
      const long long o = A.off[i], c = A.off[i + 1] - o;
      if (c > QNT_GROUP) continue;                               // the queue part's
      if (j < c) sum[l] = x[A.idx[o + j]];
      if (j == 0) row[l] = i;
    }
    group_sum_f64(sum, QNT_GROUP);
  } else {
    const long long i = A.queue[wave - gw];
    const long long o = A.off[i], c = A.off[i + 1] - o;
    LV<double> acc;
    QM_LANES(l) { double a = 0.0; for (long long k = l; k < c; k += 64) a += x[A.idx[o + k]]; acc[l] = a; }
    const double s = wave_sum_f64(acc);
    QM_LANES(l) { row[l] = l == 0 ? i : -1; sum[l] = s; }
  }
}

constexpr long long quant_side_waves(const QuantCsr& A) { return quant_group_waves(A.n) + A.nq; }

// a * b + c with both roundings (never contracted into a fused multiply-add: the device and the emulation give the same bits)
QM_DEV double quant_mul_add(double a, double b, double c) {
#ifndef QM_EMU
#pragma clang fp contract(off)
#endif
  const double p = a * b;
  return p + c;
}

QM_DEV void quant_class_wave(const QuantState& Q, long long wave) {
  LV<long long> row; LV<double> d;
  quant_row_sums(Q.cls, Q.w, wave, row, d);
  QM_LANES(l) {
    const long long c = row[l];
    if (c < 0) continue;
    const bool one = Q.cls.off[c + 1] - Q.cls.off[c] == 1;       // a single-tid class: its count goes to its transcript as it is (Q.single)
    Q.r[c] = (one || d[l] < QNT_DBL_MIN) ? 0.0 : Q.cnt[c] / d[l];
  }
}

// (the row logic keeps all 64 lanes; under VB = 1 only the lanes that finish a row evaluate E)
template <int VB>
QM_DEV void quant_txp_body(const QuantState& Q, const double* prior, long long wave) {
  LV<long long> row; LV<double> s;
  quant_row_sums(Q.txp, Q.r, wave, row, s);
  QM_LANES(l) {
    const long long t = row[l];
    if (t < 0) continue;
    const double wt = Q.w[t];
    const double a1 = quant_mul_add(wt, s[l], wt < QNT_DBL_MIN ? 0.0 : Q.single[t]);
    Q.alphaNew[t] = a1; Q.w[t] = quant_weight<VB>(a1, prior, t, Q.eff[t]);   // (w_t is read by this lane alone in this launch)
    if (Q.check && a1 > Q.minAlpha) {
      const double rel = __builtin_fabs(a1 - Q.alpha[t]) / a1;
      u64 bits; __builtin_memcpy(&bits, &rel, 8);                // rel >= 0: the bits order as the numbers do
      if (bits > Q.scal[QNT_SC_REL]) atomic_max_u64(&Q.scal[QNT_SC_REL], bits);   // (the word only ever rises: a stale read costs an atomic, no more)
    }
  }
}
QM_DEV void quant_txp_wave(const QuantState& Q, long long wave) { quant_txp_body<0>(Q, nullptr, wave); }
QM_DEV void quant_txp_vb_wave(const QuantState& Q, const double* prior, long long wave) { quant_txp_body<1>(Q, prior, wave); }

}  // namespace qm
