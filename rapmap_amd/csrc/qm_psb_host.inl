// qm_psb_host.inl -- host driver of the positional bias model (device code: qm_psb.inl; the tally half of the object:
// qm_tally_host.inl) and its pure host function, the ratios.  Included at the end of qm_host.hip: qm_psb_add reads the context's
// last result where it lies in device memory, and the transcripts' lengths are the context's replica's.  Everything above the
// extern "C" block is written against qm_exec.h and compiled twice: here, and with -DQM_EMU by tests/emu.
//
// A fold = one launch of a persistent grid, then the counters (and nothing else) read back: one host wait.  The expected counts = W
// and q up, one launch over the (transcript, bin) items, 200 words back.  The effective lengths = the list of lengths and R up, the
// tile kernel (the walk of qm_sqb.inl over this model's end biases), the per-transcript sum, eff back.  The tile table is made by the
// object's first call that needs it.  The weights are the sequence model's (qm_sqb_weights).
#include <algorithm>
#include <cmath>
#include "qm_psb.inl"
#include "qm_tally_host.inl"

struct qm_psb : qx::Tally<PSB_BINS> {
#ifndef QM_EMU
  std::shared_ptr<Replica> rep;                                       // (held while the object lives)
#endif
  SqbIdx I{};                                                         // the replica's (the emulation: the object's own) transcripts; the text is not looked at
  std::vector<u32> lens;                                              // the transcripts' lengths on the host: the overflow refusal of expect
  DevBuf<u32> d_tileCnt; DevBuf<long long> d_tileOff; long long nTiles = -1; DevBuf<unsigned char> d_tmp;   // the tile table (-1: not made yet)
  DevBuf<u64> d_W, d_P, d_q, d_exp, d_list; DevBuf<int> d_upTo; DevBuf<double> d_R, d_partial, d_eff;
  DevBuf<u32> d_qTid; DevBuf<int> d_qPos, d_qOut;                     // qm_psb_position
  int64_t lastExpectUs = 0, lastEfflenUs = 0;
  PsbIdx idx() const { return PsbIdx{I.txpLen, I.nTxp}; }
};

// (the driver's functions are what the extern "C" shells below and the emulation's face call)
static int psb_clear(qm_psb* g) {
  const int rc = g->clear();
  if (!rc) g->lastExpectUs = g->lastEfflenUs = 0;
  return rc;
}
static int psb_open(qm_psb* g) { return g->open_bins(); }
// the base's add_counts adds every count to `used`; a used fragment has two here, one of them at end 0
static int psb_add_counts(qm_psb* g, const uint64_t* obs) {
  std::vector<u64> acc(PSB_BINS + SW_C_WORDS);
  QXCHK(qx::read(g->stream, acc.data(), g->d_acc, acc.size() * sizeof(u64)));
  u64 sum = 0;
  for (int b = 0; b < PSB_BINS; ++b) { acc[(size_t)b] += obs[b]; if (b < PSB_BINS / 2) sum += obs[b]; }
  acc[PSB_BINS + SW_C_USED] += sum;
  QXCHK(qx::upload(g->stream, g->d_acc, acc.data(), acc.size() * sizeof(u64)));
  QXCHK(qx::sync(g->stream));
  memcpy(g->h, acc.data() + PSB_BINS, sizeof(g->h));
  g->units += (int64_t)sum;
  return QM_OK;
}
static int psb_fold(qm_psb* g, const UnitSrc& S, qx::Stream st) {
  return g->fold(S, st, PSB_OBS_BLOCKS_PER_CU, [&](const SweepAcc& A, int blocks) { return qx::sweep<psb_obs_wave, PSB_BINS>(st, blocks, S, g->idx(), A); });
}
static int psb_add_hits(qm_psb* g, int64_t n, const int64_t* offsets, const qm_hit* hits, int64_t maxUnits, int64_t maxHits) {
  return g->add_hits("qm_psb_add_hits", n, offsets, hits, maxUnits, maxHits, [&](const UnitSrc& S) { return psb_fold(g, S, g->stream); });
}

static int psb_stat(const qm_psb* g, int which, int64_t* value) {
  switch (which) {
    case QM_PSB_STAT_UNITS: *value = g->units; break;
    case QM_PSB_STAT_USED: *value = (int64_t)g->h[SW_C_USED]; break;
    case QM_PSB_STAT_UNMAPPED: *value = (int64_t)g->h[SW_C_UNMAPPED]; break;
    case QM_PSB_STAT_MULTI: *value = (int64_t)g->h[SW_C_MULTI]; break;
    case QM_PSB_STAT_NOT_PAIRED: *value = (int64_t)g->h[SW_C_NOT_PAIRED]; break;
    case QM_PSB_STAT_SAME_STRAND: *value = (int64_t)g->h[SW_C_SAME_STRAND]; break;
    case QM_PSB_STAT_OUT_OF_RANGE: *value = (int64_t)g->h[SW_C_OUT_OF_RANGE]; break;
    case QM_PSB_STAT_OVERHANG: *value = (int64_t)g->h[PSB_C_OVERHANG]; break;
    case QM_PSB_STAT_MAX_LEN: *value = g->maxLen; break;
    case QM_PSB_STAT_FOLDS: *value = g->folds; break;
    case QM_PSB_STAT_LAST_FOLD_US: *value = g->lastFoldUs; break;
    case QM_PSB_STAT_LAST_EXPECT_US: *value = g->lastExpectUs; break;
    case QM_PSB_STAT_LAST_EFFLEN_US: *value = g->lastEfflenUs; break;
    default: return fail(QM_E_ARG, "qm_psb_stat: unknown statistic %d", which);
  }
  return QM_OK;
}

// the tile table (gcb_tiles_wave's tiles: 64 consecutive positions of one transcript), made once
static int psb_tiles(qm_psb* g) {
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

// exp[PSB_BINS] from counts[0 .. maxLen] and q[nTxps]
static int psb_expect(qm_psb* g, const uint64_t* counts, int64_t nTxps, const uint64_t* q, uint64_t* ex) {
  if (nTxps != g->I.nTxp) return fail(QM_E_ARG, "qm_psb_expect: %lld transcripts, the index has %lld", (long long)nTxps, g->I.nTxp);
  std::vector<u64> P;
  QXCHK(sqb_prefix("qm_psb_expect", g->maxLen, counts, P));
  const unsigned __int128 lim = (unsigned __int128)1 << 63;
  const u64 Pm = P[(size_t)g->maxLen];
  unsigned __int128 w = 0;                                            // sum of q_t * L_t: below 2^128 for fewer than 2^32 transcripts
  for (int64_t t = 0; t < nTxps; ++t) w += (unsigned __int128)q[t] * g->lens[(size_t)t];
  if (Pm && w > (lim - 1) / Pm) return fail(QM_E_UNSUPPORTED, "qm_psb_expect: the weights times the lengths times the fragments reach 2^63");
  memset(ex, 0, PSB_BINS * sizeof(uint64_t));
  if (nTxps == 0) return QM_OK;
  // W[x] = W[x - 1] + P[x], x <= maxLen.  W[x] <= x P[m]: a transcript with q_t != 0 reads entries up to min(L_t, m) only, and
  // L_t P[m] < 2^63 by the refusal above; an entry beyond that may wrap -- it meets q_t == 0 alone, and a product with 0 is 0
  std::vector<u64> W(P.size(), 0);
  for (size_t x = 1; x < W.size(); ++x) W[x] = W[x - 1] + P[x];
  const qx::Stream st = g->stream;
  int rc;
  if ((rc = g->d_W.ensure((int64_t)W.size())) || (rc = g->d_q.ensure(nTxps)) || (rc = g->d_exp.ensure(PSB_BINS))) return rc;
  QXCHK(qx::upload(st, g->d_W, W.data(), W.size() * sizeof(u64)));
  QXCHK(qx::upload(st, g->d_q, q, (size_t)nTxps * sizeof(u64)));
  QXCHK(qx::fill(st, g->d_exp, 0, PSB_BINS * sizeof(u64)));
  const PsbExp E{g->idx(), g->d_W, g->d_q, g->d_exp, Pm, g->maxLen};
  QXCHK(qx::tick(g->ev0, st));
  if (Pm) HIPCHK((qx::sweep<psb_expect_wave, PSB_ACC_WORDS>(st, sweep_grid(nTxps * PSB_POS, g->numCU, PSB_EXP_BLOCKS_PER_CU, g->maxBlocks), E)));
  QXCHK(qx::tick(g->ev1, st));
  QXCHK(qx::read(st, ex, g->d_exp, PSB_BINS * sizeof(u64)));         // (waits; the tables on the host may go)
  qx::elapsed(g->ev0, g->ev1, &g->lastExpectUs);
  return QM_OK;
}

// eff[nTxps] from counts[0 .. maxLen] and R[PSB_BINS]: qm_sqb_eff_lens' steps with psb_efflen_wave as the tile kernel
static int psb_eff_lens(qm_psb* g, const uint64_t* counts, int64_t nTxps, const double* R, double* eff) {
  if (nTxps != g->I.nTxp) return fail(QM_E_ARG, "qm_psb_eff_lens: %lld transcripts, the index has %lld", (long long)nTxps, g->I.nTxp);
  std::vector<u64> P;
  QXCHK(sqb_prefix("qm_psb_eff_lens", g->maxLen, counts, P));
  if (nTxps == 0) return QM_OK;
  std::vector<u64> list; std::vector<int> upTo((size_t)g->maxLen + 1, 0);   // the lengths with counts: (the bits of (double)counts[l], l), ascending
  for (int l = 1; l <= g->maxLen; ++l) {
    if (counts[l]) { const double c = (double)counts[l]; u64 b; memcpy(&b, &c, 8); list.push_back(b); list.push_back((u64)l); }
    upTo[(size_t)l] = (int)(list.size() / 2);
  }
  list.push_back(0); list.push_back(0);                               // (never empty; behind what upTo counts)
  const qx::Stream st = g->stream;
  int rc;
  QXCHK(psb_tiles(g));
  if ((rc = g->d_P.ensure((int64_t)P.size())) || (rc = g->d_list.ensure((int64_t)list.size())) || (rc = g->d_upTo.ensure((int64_t)upTo.size())) || (rc = g->d_R.ensure(PSB_BINS)) ||
      (rc = g->d_partial.ensure(std::max<long long>(g->nTiles, 1))) || (rc = g->d_eff.ensure(nTxps))) return rc;
  QXCHK(qx::upload(st, g->d_P, P.data(), P.size() * sizeof(u64)));
  QXCHK(qx::upload(st, g->d_list, list.data(), list.size() * sizeof(u64)));
  QXCHK(qx::upload(st, g->d_upTo, upTo.data(), upTo.size() * sizeof(int)));
  QXCHK(qx::upload(st, g->d_R, R, PSB_BINS * sizeof(double)));
  const SqbEff E{g->I, g->d_tileOff, g->d_list, g->d_upTo, g->d_R, g->d_partial, g->nTiles, g->maxLen};
  QXCHK(qx::tick(g->ev0, st));
  if (g->nTiles > 0)
    HIPCHK((qx::sweep<psb_efflen_wave, SQB_RING_WORDS>(st, sweep_grid(g->nTiles * 64, g->numCU, SQB_BLOCKS_PER_CU, g->maxBlocks), E)));
  HIPCHK((qx::launch<sqb_tilesum_wave>(st, qx::waves_of(nTxps), g->I.txpLen, (const long long*)g->d_tileOff.p, (const double*)g->d_partial.p, (const u64*)g->d_P.p,
                                       g->maxLen, (long long)nTxps, g->d_eff.p)));
  QXCHK(qx::tick(g->ev1, st));
  QXCHK(qx::read(st, eff, g->d_eff, (size_t)nTxps * sizeof(double)));  // (waits; the tables on the host may go)
  qx::elapsed(g->ev0, g->ev1, &g->lastEfflenUs);
  return QM_OK;
}

static int psb_position(qm_psb* g, int64_t n, const uint32_t* tids, const int32_t* pos, int32_t* out) {
  if (n <= 0) return QM_OK;
  const qx::Stream st = g->stream;
  int rc;
  if ((rc = g->d_qTid.ensure(n)) || (rc = g->d_qPos.ensure(n)) || (rc = g->d_qOut.ensure(n * 2))) return rc;
  QXCHK(qx::upload(st, g->d_qTid, tids, (size_t)n * 4)); QXCHK(qx::upload(st, g->d_qPos, pos, (size_t)n * 4));
  HIPCHK((qx::launch<psb_probe_wave>(st, qx::waves_of(n), g->idx(), (long long)n, (const u32*)g->d_qTid.p, (const int*)g->d_qPos.p, g->d_qOut.p)));
  return qx::read(st, out, g->d_qOut, (size_t)n * 2 * 4);
}

// ---- the pure host function (include/qmap_mi355.h: RATIOS); every operation on its own, nothing fused
static int psb_ratios(const uint64_t* obs, const uint64_t* ex, double* R) {
#ifndef QM_EMU
#pragma clang fp contract(off)
#endif
  if (!obs || !ex || !R) return fail(QM_E_ARG, "qm_psb_ratios: bad argument");
  for (int row = 0; row < PSB_BINS; row += PSB_POS) {                 // an (end, class)
    u64 so = 0, se = 0;
    for (int b = 0; b < PSB_POS; ++b) { so += obs[row + b]; se += ex[row + b]; }
    for (int b = 0; b < PSB_POS; ++b) {
      if (!so || !se) { R[row + b] = 1.0; continue; }
      const double po = (double)(obs[row + b] + 1) / (double)(so + PSB_POS), pe = (double)(ex[row + b] + 1) / (double)(se + PSB_POS);
      double r = po / pe;
      if (r < 0.25) r = 0.25;
      if (r > 4.0) r = 4.0;
      R[row + b] = r;
    }
  }
  return QM_OK;
}

#ifndef QM_EMU
extern "C" {

int qm_psb_ratios(const uint64_t* obs, const uint64_t* exp, double* R) { return psb_ratios(obs, exp, R); }

int qm_psb_create(qm_ctx* c, int32_t max_len, uint32_t flags, qm_psb** out) {
  if (!c || !out || (flags & ~0xffffu)) return fail(QM_E_ARG, "qm_psb_create: bad argument");
  if (max_len < 1) return fail(QM_E_ARG, "qm_psb_create: max_len %d", (int)max_len);
  if (max_len > SQB_MAX_LEN) return fail(QM_E_UNSUPPORTED, "qm_psb_create: max_len %d beyond %d", (int)max_len, SQB_MAX_LEN);
  HIPCHK(hipSetDevice(c->device));
  qm_psb* g = new qm_psb();
  g->maxLen = max_len; g->maxBlocks = (int)(flags & 0xffffu);
  g->lens.resize((size_t)c->ix->nTxp);
  for (int64_t t = 0; t < c->ix->nTxp; ++t) g->lens[(size_t)t] = (u32)c->ix->lens[(size_t)t];
  int rc = g->open("qm_psb_create", c->device, c->numCU);
  if (!rc && psb_open(g) != QM_OK) rc = fail(QM_E_NOGPU, "qm_psb_create: bins");
  if (rc) { qm_psb_destroy(g); return rc; }
  g->rep = c->rep;
  g->I = SqbIdx{c->rep->text, c->rep->txpOff, c->rep->txpLen, c->ix->nTxp, c->ix->n};
  *out = g;
  return QM_OK;
}

int qm_psb_destroy(qm_psb* g) {
  if (!g) return QM_OK;
  g->close();
  delete g;                    // (the buffers free themselves; the replica lives while an object holds it)
  return QM_OK;
}

int qm_psb_clear(qm_psb* g) {
  QXCHK(qx::enter(g, true, "null object"));
  return psb_clear(g);
}

int qm_psb_add(qm_psb* g, qm_ctx* c) {
  QXCHK(qx::enter_add(g, c, "qm_psb_add", "positional-bias counts", "sweep"));
  if (c->rep.get() != g->rep.get()) return fail(QM_E_ARG, "qm_psb_add: the context maps to another index");
  return psb_fold(g, qx::last_units(c), c->stream);
}

int qm_psb_add_hits(qm_psb* g, int64_t n, const int64_t* offsets, const qm_hit* hits) {
  QXCHK(qx::enter(g, true, "qm_psb_add_hits: bad argument"));
  return psb_add_hits(g, n, offsets, hits, 1 << 22, 1 << 21);       // a part: what is uploaded and swept in one go
}

int qm_psb_fetch(qm_psb* g, uint64_t* obs) {
  QXCHK(qx::enter(g, obs != nullptr, "qm_psb_fetch: bad argument"));
  return g->fetch(obs, PSB_BINS);
}

int qm_psb_add_counts(qm_psb* g, const uint64_t* obs) {
  QXCHK(qx::enter(g, obs != nullptr, "qm_psb_add_counts: bad argument"));
  return psb_add_counts(g, obs);
}

int qm_psb_stat(const qm_psb* g, int which, int64_t* value) {
  if (!g || !value) return fail(QM_E_ARG, "qm_psb_stat: bad argument");
  return psb_stat(g, which, value);
}

int qm_psb_expect(qm_psb* g, const uint64_t* counts, int64_t n_txps, const uint64_t* q, uint64_t* exp) {
  QXCHK(qx::enter(g, counts && exp && n_txps >= 0 && (n_txps == 0 || q), "qm_psb_expect: bad argument"));
  return psb_expect(g, counts, n_txps, q, exp);
}

int qm_psb_eff_lens(qm_psb* g, const uint64_t* counts, int64_t n_txps, const double* R, double* eff) {
  QXCHK(qx::enter(g, counts && R && n_txps >= 0 && (n_txps == 0 || eff), "qm_psb_eff_lens: bad argument"));
  return psb_eff_lens(g, counts, n_txps, R, eff);
}

int qm_psb_position(qm_psb* g, int64_t n, const uint32_t* tids, const int32_t* positions, int32_t* out) {
  QXCHK(qx::enter(g, n >= 0 && (n == 0 || (tids && positions && out)), "qm_psb_position: bad argument"));
  return psb_position(g, n, tids, positions, out);
}

}  // extern "C"
#endif
