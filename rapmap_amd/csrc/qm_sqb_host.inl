// qm_sqb_host.inl -- host driver of the sequence-specific bias model (device code: qm_sqb.inl; the tally half of the object:
// qm_tally_host.inl) and its two pure host functions, the weights and the ratios.  Included at the end of qm_host.hip: qm_sqb_add
// reads the context's last result where it lies in device memory, and the text is the context's replica's.  Everything above the
// extern "C" block is written against qm_exec.h and compiled twice: here, and with -DQM_EMU by tests/emu.
//
// A fold = one launch of a persistent grid, then the eight counters (and nothing else) read back: one host wait.  The expected
// counts = P and q up, one launch over the tile table, 1152 words back.  The effective lengths = the list of lengths and R up, the tile
// kernel, the per-transcript sum, eff back.  The tile table is made by the object's first call that needs it.
#include <algorithm>
#include <cmath>
#include "qm_sqb.inl"
#include "qm_tally_host.inl"

struct qm_sqb : qx::Tally<SQB_BINS> {
#ifndef QM_EMU
  std::shared_ptr<Replica> rep;                                       // (held while the object lives)
#endif
  SqbIdx I{};                                                         // the replica's (the emulation: the object's own) text and transcripts
  std::vector<u32> lens;                                              // the transcripts' lengths on the host: the overflow refusal of expect
  DevBuf<u32> d_tileCnt; DevBuf<long long> d_tileOff; long long nTiles = -1; DevBuf<unsigned char> d_tmp;   // the tile table (-1: not made yet)
  DevBuf<u64> d_P, d_q, d_exp, d_list; DevBuf<int> d_upTo; DevBuf<double> d_R, d_partial, d_eff;
  DevBuf<u32> d_qTid; DevBuf<int> d_qPos, d_qEnd, d_qOut;             // qm_sqb_context
  int64_t lastExpectUs = 0, lastEfflenUs = 0;
};

// (the driver's functions are what the extern "C" shells below and the emulation's face call)
static int sqb_clear(qm_sqb* g) {
  const int rc = g->clear();
  if (!rc) g->lastExpectUs = g->lastEfflenUs = 0;
  return rc;
}
static int sqb_open(qm_sqb* g) { return g->open_bins(); }
// the base's add_counts adds every count to `used`; a used fragment has 18 here, one of them in the first 64 entries
static int sqb_add_counts(qm_sqb* g, const uint64_t* obs) {
  std::vector<u64> acc(SQB_BINS + SW_C_WORDS);
  QXCHK(qx::read(g->stream, acc.data(), g->d_acc, acc.size() * sizeof(u64)));
  u64 sum = 0;
  for (int b = 0; b < SQB_BINS; ++b) { acc[(size_t)b] += obs[b]; if (b < 64) sum += obs[b]; }
  acc[SQB_BINS + SW_C_USED] += sum;
  QXCHK(qx::upload(g->stream, g->d_acc, acc.data(), acc.size() * sizeof(u64)));
  QXCHK(qx::sync(g->stream));
  memcpy(g->h, acc.data() + SQB_BINS, sizeof(g->h));
  g->units += (int64_t)sum;
  return QM_OK;
}
static int sqb_fold(qm_sqb* g, const UnitSrc& S, qx::Stream st) {
  return g->fold(S, st, SQB_OBS_BLOCKS_PER_CU, [&](const SweepAcc& A, int blocks) { return qx::sweep<sqb_obs_wave, SQB_BINS>(st, blocks, S, g->I, A); });
}
static int sqb_add_hits(qm_sqb* g, int64_t n, const int64_t* offsets, const qm_hit* hits, int64_t maxUnits, int64_t maxHits) {
  return g->add_hits("qm_sqb_add_hits", n, offsets, hits, maxUnits, maxHits, [&](const UnitSrc& S) { return sqb_fold(g, S, g->stream); });
}

static int sqb_stat(const qm_sqb* g, int which, int64_t* value) {
  switch (which) {
    case QM_SQB_STAT_UNITS: *value = g->units; break;
    case QM_SQB_STAT_USED: *value = (int64_t)g->h[SW_C_USED]; break;
    case QM_SQB_STAT_UNMAPPED: *value = (int64_t)g->h[SW_C_UNMAPPED]; break;
    case QM_SQB_STAT_MULTI: *value = (int64_t)g->h[SW_C_MULTI]; break;
    case QM_SQB_STAT_NOT_PAIRED: *value = (int64_t)g->h[SW_C_NOT_PAIRED]; break;
    case QM_SQB_STAT_SAME_STRAND: *value = (int64_t)g->h[SW_C_SAME_STRAND]; break;
    case QM_SQB_STAT_OUT_OF_RANGE: *value = (int64_t)g->h[SW_C_OUT_OF_RANGE]; break;
    case QM_SQB_STAT_OVERHANG: *value = (int64_t)g->h[SQB_C_OVERHANG]; break;
    case QM_SQB_STAT_AMBIGUOUS: *value = (int64_t)g->h[SQB_C_AMBIGUOUS]; break;
    case QM_SQB_STAT_MAX_LEN: *value = g->maxLen; break;
    case QM_SQB_STAT_FOLDS: *value = g->folds; break;
    case QM_SQB_STAT_LAST_FOLD_US: *value = g->lastFoldUs; break;
    case QM_SQB_STAT_LAST_EXPECT_US: *value = g->lastExpectUs; break;
    case QM_SQB_STAT_LAST_EFFLEN_US: *value = g->lastEfflenUs; break;
    default: return fail(QM_E_ARG, "qm_sqb_stat: unknown statistic %d", which);
  }
  return QM_OK;
}

// P[d] = fragments of length <= d, d = 0 .. maxLen
static int sqb_prefix(const char* who, int maxLen, const uint64_t* counts, std::vector<u64>& P) {
  if (counts[0]) return fail(QM_E_ARG, "%s: bin 0 holds %llu", who, (unsigned long long)counts[0]);
  P.assign((size_t)maxLen + 1, 0);
  for (int l = 1; l <= maxLen; ++l) {
    if (counts[l] >= (1ULL << 63) - P[(size_t)l - 1]) return fail(QM_E_UNSUPPORTED, "%s: 2^63 fragments or more", who);
    P[(size_t)l] = P[(size_t)l - 1] + counts[l];
  }
  return QM_OK;
}

// the tile table (gcb_tiles_wave's tiles: 64 consecutive positions of one transcript), made once
static int sqb_tiles(qm_sqb* g) {
  if (g->nTiles >= 0) return QM_OK;
  const qx::Stream st = g->stream; const long long nTxp = g->I.nTxp;
  int rc;
  if ((rc = g->d_tileCnt.ensure(nTxp + 1)) || (rc = g->d_tileOff.ensure(nTxp + 1))) return rc;
  HIPCHK((qx::launch<gcb_tiles_wave>(st, qx::waves_of(nTxp + 1), g->I.txpLen, nTxp, g->d_tileCnt.p)));
  QXCHK(qx::scan_u32(st, g->d_tmp, g->d_tileCnt, g->d_tileOff, nTxp + 1));
  long long total = 0;
  QXCHK(qx::read(st, &total, g->d_tileOff + nTxp, sizeof(total)));
  g->nTiles = total;
  return QM_OK;
}

// exp[SQB_BINS] from counts[0 .. maxLen] and q[nTxps]
static int sqb_expect(qm_sqb* g, const uint64_t* counts, int64_t nTxps, const uint64_t* q, uint64_t* ex) {
  if (nTxps != g->I.nTxp) return fail(QM_E_ARG, "qm_sqb_expect: %lld transcripts, the index has %lld", (long long)nTxps, g->I.nTxp);
  std::vector<u64> P;
  QXCHK(sqb_prefix("qm_sqb_expect", g->maxLen, counts, P));
  const unsigned __int128 lim = (unsigned __int128)1 << 63;
  const u64 Pm = P[(size_t)g->maxLen];
  unsigned __int128 w = 0;                                            // sum of q_t * L_t: below 2^128 for fewer than 2^32 transcripts
  for (int64_t t = 0; t < nTxps; ++t) w += (unsigned __int128)q[t] * g->lens[(size_t)t];
  if (Pm && w > (lim - 1) / Pm) return fail(QM_E_UNSUPPORTED, "qm_sqb_expect: the weights times the lengths times the fragments reach 2^63");
  memset(ex, 0, SQB_BINS * sizeof(uint64_t));
  if (nTxps == 0) return QM_OK;
  const qx::Stream st = g->stream;
  int rc;
  QXCHK(sqb_tiles(g));
  if ((rc = g->d_P.ensure((int64_t)P.size())) || (rc = g->d_q.ensure(nTxps)) || (rc = g->d_exp.ensure(SQB_BINS))) return rc;
  QXCHK(qx::upload(st, g->d_P, P.data(), P.size() * sizeof(u64)));
  QXCHK(qx::upload(st, g->d_q, q, (size_t)nTxps * sizeof(u64)));
  QXCHK(qx::fill(st, g->d_exp, 0, SQB_BINS * sizeof(u64)));
  const SqbExp E{g->I, g->d_tileOff, g->d_P, g->d_q, g->d_exp, g->nTiles, g->maxLen};
  QXCHK(qx::tick(g->ev0, st));
  if (Pm && g->nTiles > 0)
    HIPCHK((qx::sweep<sqb_expect_wave, SQB_ACC_WORDS>(st, sweep_grid(g->nTiles * 64, g->numCU, SQB_BLOCKS_PER_CU, g->maxBlocks), E)));
  QXCHK(qx::tick(g->ev1, st));
  QXCHK(qx::read(st, ex, g->d_exp, SQB_BINS * sizeof(u64)));         // (waits; the tables on the host may go)
  qx::elapsed(g->ev0, g->ev1, &g->lastExpectUs);
  return QM_OK;
}

// eff[nTxps] from counts[0 .. maxLen] and R[SQB_BINS]
static int sqb_eff_lens(qm_sqb* g, const uint64_t* counts, int64_t nTxps, const double* R, double* eff) {
  if (nTxps != g->I.nTxp) return fail(QM_E_ARG, "qm_sqb_eff_lens: %lld transcripts, the index has %lld", (long long)nTxps, g->I.nTxp);
  std::vector<u64> P;
  QXCHK(sqb_prefix("qm_sqb_eff_lens", g->maxLen, counts, P));
  if (nTxps == 0) return QM_OK;
  std::vector<u64> list; std::vector<int> upTo((size_t)g->maxLen + 1, 0);   // the lengths with counts: (the bits of (double)counts[l], l), ascending
  for (int l = 1; l <= g->maxLen; ++l) {
    if (counts[l]) { const double c = (double)counts[l]; u64 b; memcpy(&b, &c, 8); list.push_back(b); list.push_back((u64)l); }
    upTo[(size_t)l] = (int)(list.size() / 2);
  }
  list.push_back(0); list.push_back(0);                               // (never empty; behind what upTo counts)
  const qx::Stream st = g->stream;
  int rc;
  QXCHK(sqb_tiles(g));
  if ((rc = g->d_P.ensure((int64_t)P.size())) || (rc = g->d_list.ensure((int64_t)list.size())) || (rc = g->d_upTo.ensure((int64_t)upTo.size())) || (rc = g->d_R.ensure(SQB_BINS)) ||
      (rc = g->d_partial.ensure(std::max<long long>(g->nTiles, 1))) || (rc = g->d_eff.ensure(nTxps))) return rc;
  QXCHK(qx::upload(st, g->d_P, P.data(), P.size() * sizeof(u64)));
  QXCHK(qx::upload(st, g->d_list, list.data(), list.size() * sizeof(u64)));
  QXCHK(qx::upload(st, g->d_upTo, upTo.data(), upTo.size() * sizeof(int)));
  QXCHK(qx::upload(st, g->d_R, R, SQB_BINS * sizeof(double)));
  const SqbEff E{g->I, g->d_tileOff, g->d_list, g->d_upTo, g->d_R, g->d_partial, g->nTiles, g->maxLen};
  QXCHK(qx::tick(g->ev0, st));
  if (g->nTiles > 0)
    HIPCHK((qx::sweep<sqb_efflen_wave, SQB_RING_WORDS>(st, sweep_grid(g->nTiles * 64, g->numCU, SQB_BLOCKS_PER_CU, g->maxBlocks), E)));
  HIPCHK((qx::launch<sqb_tilesum_wave>(st, qx::waves_of(nTxps), g->I.txpLen, (const long long*)g->d_tileOff.p, (const double*)g->d_partial.p, (const u64*)g->d_P.p,
                                       g->maxLen, (long long)nTxps, g->d_eff.p)));
  QXCHK(qx::tick(g->ev1, st));
  QXCHK(qx::read(st, eff, g->d_eff, (size_t)nTxps * sizeof(double)));  // (waits; the tables on the host may go)
  qx::elapsed(g->ev0, g->ev1, &g->lastEfflenUs);
  return QM_OK;
}

static int sqb_context(qm_sqb* g, int64_t n, const uint32_t* tids, const int32_t* pos, const int32_t* ends, int32_t* out) {
  if (n <= 0) return QM_OK;
  const qx::Stream st = g->stream;
  int rc;
  if ((rc = g->d_qTid.ensure(n)) || (rc = g->d_qPos.ensure(n)) || (rc = g->d_qEnd.ensure(n)) || (rc = g->d_qOut.ensure(n * SQB_CTX))) return rc;
  QXCHK(qx::upload(st, g->d_qTid, tids, (size_t)n * 4)); QXCHK(qx::upload(st, g->d_qPos, pos, (size_t)n * 4)); QXCHK(qx::upload(st, g->d_qEnd, ends, (size_t)n * 4));
  HIPCHK((qx::launch<sqb_probe_wave>(st, qx::waves_of(n), g->I, (long long)n, (const u32*)g->d_qTid.p, (const int*)g->d_qPos.p, (const int*)g->d_qEnd.p, g->d_qOut.p)));
  return qx::read(st, out, g->d_qOut, (size_t)n * SQB_CTX * 4);
}

// ---- the two pure host functions (include/qmap_mi355.h: WEIGHTS, RATIOS); every operation on its own, nothing fused
static int sqb_weights(int32_t maxLen, const uint64_t* counts, int64_t nTxps, const uint32_t* lens, const double* alpha, uint64_t* q, int32_t* kOut) {
#ifndef QM_EMU
#pragma clang fp contract(off)
#endif
  if (maxLen < 1) return fail(QM_E_ARG, "qm_sqb_weights: max_len %d", (int)maxLen);
  if (maxLen > SQB_MAX_LEN) return fail(QM_E_UNSUPPORTED, "qm_sqb_weights: max_len %d beyond %d", (int)maxLen, SQB_MAX_LEN);
  if (!counts || !kOut || nTxps < 0 || (nTxps > 0 && (!lens || !alpha || !q))) return fail(QM_E_ARG, "qm_sqb_weights: bad argument");
  std::vector<u64> P;
  QXCHK(sqb_prefix("qm_sqb_weights", maxLen, counts, P));
  std::vector<u64> Q((size_t)maxLen + 1, 0);                          // (an entry beyond min(L, max_len) of the longest transcript may wrap: never read)
  for (int l = 1; l <= maxLen; ++l) Q[(size_t)l] = Q[(size_t)l - 1] + (u64)l * counts[l];
  const u64 Pm = P[(size_t)maxLen];
  u64 maxL = 0;
  for (int64_t t = 0; t < nTxps; ++t) {
    if (!lens[t]) return fail(QM_E_ARG, "qm_sqb_weights: transcript %lld has length 0", (long long)t);
    maxL = std::max<u64>(maxL, lens[t]);
  }
  if (Pm && maxL + 1 > ((1ULL << 63) - 1) / Pm) return fail(QM_E_UNSUPPORTED, "qm_sqb_weights: fragments times the longest transcript reach 2^63");
  std::vector<double> rho((size_t)nTxps, 0.0);
  double X = 0.0;
  for (int64_t t = 0; t < nTxps; ++t) {
    const u64 L = lens[t], mm = std::min<u64>(L, (u64)maxLen);
    const u64 S = (L + 1) * P[(size_t)mm] - Q[(size_t)mm];
    if (alpha[t] > 0.0 && S) rho[(size_t)t] = alpha[t] / (double)S;
    const double w = rho[(size_t)t] * (double)L;
    X = X + w;
  }
  const double z = X * (double)Pm;
  if (!(z == z) || std::isinf(z)) return fail(QM_E_ARG, "qm_sqb_weights: the estimate is not finite");
  if (z == 0.0) {
    for (int64_t t = 0; t < nTxps; ++t) q[t] = 0;
    *kOut = 0;
    return QM_OK;
  }
  const int k = 61 - std::ilogb(z);
  for (int64_t t = 0; t < nTxps; ++t) q[t] = (uint64_t)std::floor(std::ldexp(rho[(size_t)t], k));
  *kOut = k;
  return QM_OK;
}

static int sqb_ratios(const uint64_t* obs, const uint64_t* ex, double* R) {
#ifndef QM_EMU
#pragma clang fp contract(off)
#endif
  if (!obs || !ex || !R) return fail(QM_E_ARG, "qm_sqb_ratios: bad argument");
  for (int e = 0; e < 2; ++e) for (int j = 0; j < SQB_CTX; ++j) {
    const int row = (e * SQB_CTX + j) * 64, words = j == 0 ? 4 : j == 1 ? 16 : 64;
    for (int w = 0; w < 64; ++w) {
      if (w >= words) { R[row + w] = 1.0; continue; }
      const int g0 = row + (w & ~3);
      const u64 so = obs[g0] + obs[g0 + 1] + obs[g0 + 2] + obs[g0 + 3], se = ex[g0] + ex[g0 + 1] + ex[g0 + 2] + ex[g0 + 3];
      const double po = (double)(obs[row + w] + 1) / (double)(so + 4), pe = (double)(ex[row + w] + 1) / (double)(se + 4);
      double r = po / pe;
      if (r < 0.25) r = 0.25;
      if (r > 4.0) r = 4.0;
      R[row + w] = r;
    }
  }
  return QM_OK;
}

#ifndef QM_EMU
extern "C" {

int qm_sqb_weights(int32_t max_len, const uint64_t* counts, int64_t n_txps, const uint32_t* lens, const double* alpha, uint64_t* q, int32_t* k) {
  return sqb_weights(max_len, counts, n_txps, lens, alpha, q, k);
}

int qm_sqb_ratios(const uint64_t* obs, const uint64_t* exp, double* R) { return sqb_ratios(obs, exp, R); }

int qm_sqb_create(qm_ctx* c, int32_t max_len, uint32_t flags, qm_sqb** out) {
  if (!c || !out || (flags & ~0xffffu)) return fail(QM_E_ARG, "qm_sqb_create: bad argument");
  if (max_len < 1) return fail(QM_E_ARG, "qm_sqb_create: max_len %d", (int)max_len);
  if (max_len > SQB_MAX_LEN) return fail(QM_E_UNSUPPORTED, "qm_sqb_create: max_len %d beyond %d", (int)max_len, SQB_MAX_LEN);
  HIPCHK(hipSetDevice(c->device));
  qm_sqb* g = new qm_sqb();
  g->maxLen = max_len; g->maxBlocks = (int)(flags & 0xffffu);
  g->lens.resize((size_t)c->ix->nTxp);
  for (int64_t t = 0; t < c->ix->nTxp; ++t) g->lens[(size_t)t] = (u32)c->ix->lens[(size_t)t];
  int rc = g->open("qm_sqb_create", c->device, c->numCU);
  if (!rc && sqb_open(g) != QM_OK) rc = fail(QM_E_NOGPU, "qm_sqb_create: bins");
  if (rc) { qm_sqb_destroy(g); return rc; }
  g->rep = c->rep;
  g->I = SqbIdx{c->rep->text, c->rep->txpOff, c->rep->txpLen, c->ix->nTxp, c->ix->n};
  *out = g;
  return QM_OK;
}

int qm_sqb_destroy(qm_sqb* g) {
  if (!g) return QM_OK;
  g->close();
  delete g;                    // (the buffers free themselves; the replica lives while an object holds it)
  return QM_OK;
}

int qm_sqb_clear(qm_sqb* g) {
  QXCHK(qx::enter(g, true, "null object"));
  return sqb_clear(g);
}

int qm_sqb_add(qm_sqb* g, qm_ctx* c) {
  QXCHK(qx::enter_add(g, c, "qm_sqb_add", "sequence-bias counts", "sweep"));
  if (c->rep.get() != g->rep.get()) return fail(QM_E_ARG, "qm_sqb_add: the context maps to another index");
  return sqb_fold(g, qx::last_units(c), c->stream);
}

int qm_sqb_add_hits(qm_sqb* g, int64_t n, const int64_t* offsets, const qm_hit* hits) {
  QXCHK(qx::enter(g, true, "qm_sqb_add_hits: bad argument"));
  return sqb_add_hits(g, n, offsets, hits, 1 << 22, 1 << 21);       // a part: what is uploaded and swept in one go
}

int qm_sqb_fetch(qm_sqb* g, uint64_t* obs) {
  QXCHK(qx::enter(g, obs != nullptr, "qm_sqb_fetch: bad argument"));
  return g->fetch(obs, SQB_BINS);
}

int qm_sqb_add_counts(qm_sqb* g, const uint64_t* obs) {
  QXCHK(qx::enter(g, obs != nullptr, "qm_sqb_add_counts: bad argument"));
  return sqb_add_counts(g, obs);
}

int qm_sqb_stat(const qm_sqb* g, int which, int64_t* value) {
  if (!g || !value) return fail(QM_E_ARG, "qm_sqb_stat: bad argument");
  return sqb_stat(g, which, value);
}

int qm_sqb_expect(qm_sqb* g, const uint64_t* counts, int64_t n_txps, const uint64_t* q, uint64_t* exp) {
  QXCHK(qx::enter(g, counts && exp && n_txps >= 0 && (n_txps == 0 || q), "qm_sqb_expect: bad argument"));
  return sqb_expect(g, counts, n_txps, q, exp);
}

int qm_sqb_eff_lens(qm_sqb* g, const uint64_t* counts, int64_t n_txps, const double* R, double* eff) {
  QXCHK(qx::enter(g, counts && R && n_txps >= 0 && (n_txps == 0 || eff), "qm_sqb_eff_lens: bad argument"));
  return sqb_eff_lens(g, counts, n_txps, R, eff);
}

int qm_sqb_context(qm_sqb* g, int64_t n, const uint32_t* tids, const int32_t* positions, const int32_t* ends, int32_t* out) {
  QXCHK(qx::enter(g, n >= 0 && (n == 0 || (tids && positions && ends && out)), "qm_sqb_context: bad argument"));
  return sqb_context(g, n, tids, positions, ends, out);
}

}  // extern "C"
#endif
