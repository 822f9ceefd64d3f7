// qm_gcb_host.inl -- host driver of the fragment GC bias model (device code: qm_gcb.inl; the tally half of the object:
// qm_tally_host.inl) and the arithmetic from the two sets of counts to effective lengths.  Included at the end of qm_host.hip:
// qm_gcb_add reads the context's last result where it lies in device memory, and the rank structure lives in the context's
// replica.  Everything above the extern "C" block is written against qm_exec.h and compiled twice: here, and with -DQM_EMU by
// tests/emu.
//
// A fold = one launch of a persistent grid, then the seven counters (and nothing else) read back: one host wait.  The expected
// matrix = the table of (count, reciprocal) per length up, one launch over the tile table, H back.  The tile table is made by the
// object's first qm_gcb_expect.
#include <algorithm>
#include "qm_gcb.inl"
#include "qm_tally_host.inl"

struct qm_gcb : qx::Tally<GCB_SLAB> {
#ifndef QM_EMU
  std::shared_ptr<Replica> rep;                                       // (held while the object lives; the base's buffers are freed after it is released and need nothing from it)
#endif
  GcbIdx I{};                                                         // the replica's (the emulation: the object's own) rank structure and transcripts
  long long maxTxpLen = 0;                                            // the longest transcript: the overflow refusal of expect
  DevBuf<u32> d_tileCnt; DevBuf<long long> d_tileOff; long long nTiles = -1;   // the tile table (-1: not made yet)
  DevBuf<u64> d_tab, d_H; DevBuf<unsigned char> d_tmp;                // expect: (count, reciprocal) per length, the matrix, the scan's scratch
  DevBuf<u32> d_qTid; DevBuf<int> d_qStart, d_qLen, d_qOut;           // qm_gcb_window_gc
  int64_t lastExpectUs = 0, rankBuildUs = 0;
};

// The rank structure over text[0 .. n) into mask and rank (gcb_blocks(n) words each); tmp: scratch.  The stream is idle when this returns.
static int gcb_build_rank(qx::Stream st, const unsigned char* text, long long n, DevBuf<u64>& mask, DevBuf<u32>& rank, DevBuf<unsigned char>& tmp) {
  const long long nBlk = gcb_blocks(n);
  DevBuf<u32> cnt; DevBuf<long long> scan;
  int rc;
  if ((rc = mask.ensure(nBlk)) || (rc = rank.ensure(nBlk)) || (rc = cnt.ensure(nBlk)) || (rc = scan.ensure(nBlk))) return rc;
  HIPCHK((qx::launch<gcb_mask_wave>(st, qx::waves_of(nBlk), text, n, nBlk, mask.p, cnt.p)));
  QXCHK(qx::scan_u32(st, tmp, cnt, scan, nBlk));
  HIPCHK((qx::launch<gcb_rank_wave>(st, qx::waves_of(nBlk), (const long long*)scan.p, nBlk, rank.p)));
  return qx::sync(st);                                                // (cnt and scan go out of scope)
}

// (the driver's functions are what the extern "C" shells below and the emulation's face call)
static int gcb_clear(qm_gcb* g) {
  const int rc = g->clear();
  if (!rc) g->lastExpectUs = 0;
  return rc;
}
static int gcb_open(qm_gcb* g) { return g->open_bins(); }
static int gcb_add_counts(qm_gcb* g, const uint64_t* obs) { return g->add_counts(obs, GCB_BINS); }
static int gcb_fold(qm_gcb* g, const UnitSrc& S, qx::Stream st) {
  return g->fold(S, st, GCB_BLOCKS_PER_CU, [&](const SweepAcc& A, int blocks) { return qx::sweep<gcb_obs_wave, GCB_SLAB>(st, blocks, S, g->I, A); });
}
// qm_gcb_add_hits: the host arrays in parts (at most maxUnits units and maxHits hits each) through the fold
static int gcb_add_hits(qm_gcb* g, int64_t n, const int64_t* offsets, const qm_hit* hits, int64_t maxUnits, int64_t maxHits) {
  return g->add_hits("qm_gcb_add_hits", n, offsets, hits, maxUnits, maxHits, [&](const UnitSrc& S) { return gcb_fold(g, S, g->stream); });
}

static int gcb_stat(const qm_gcb* g, int which, int64_t* value) {
  switch (which) {
    case QM_GCB_STAT_UNITS: *value = g->units; break;
    case QM_GCB_STAT_USED: *value = (int64_t)g->h[SW_C_USED]; break;
    case QM_GCB_STAT_UNMAPPED: *value = (int64_t)g->h[SW_C_UNMAPPED]; break;
    case QM_GCB_STAT_MULTI: *value = (int64_t)g->h[SW_C_MULTI]; break;
    case QM_GCB_STAT_NOT_PAIRED: *value = (int64_t)g->h[SW_C_NOT_PAIRED]; break;
    case QM_GCB_STAT_SAME_STRAND: *value = (int64_t)g->h[SW_C_SAME_STRAND]; break;
    case QM_GCB_STAT_OUT_OF_RANGE: *value = (int64_t)g->h[SW_C_OUT_OF_RANGE]; break;
    case QM_GCB_STAT_OVERHANG: *value = (int64_t)g->h[GCB_C_OVERHANG]; break;
    case QM_GCB_STAT_MAX_LEN: *value = g->maxLen; break;
    case QM_GCB_STAT_FOLDS: *value = g->folds; break;
    case QM_GCB_STAT_LAST_FOLD_US: *value = g->lastFoldUs; break;
    case QM_GCB_STAT_LAST_EXPECT_US: *value = g->lastExpectUs; break;
    case QM_GCB_STAT_RANK_BUILD_US: *value = g->rankBuildUs; break;
    default: return fail(QM_E_ARG, "qm_gcb_stat: unknown statistic %d", which);
  }
  return QM_OK;
}

// H[n_txps][GCB_BINS] from counts[0 .. maxLen]
static int gcb_expect(qm_gcb* g, const uint64_t* counts, int64_t nTxps, uint64_t* H) {
  if (nTxps != g->I.nTxp) return fail(QM_E_ARG, "qm_gcb_expect: %lld transcripts, the index has %lld", (long long)nTxps, g->I.nTxp);
  if (counts[0]) return fail(QM_E_ARG, "qm_gcb_expect: bin 0 holds %llu", (unsigned long long)counts[0]);
  const u64 lim = 1ULL << 63;
  u64 P = 0;
  std::vector<u64> tab(2 * ((size_t)g->maxLen + 1), 0);
  for (int l = 1; l <= g->maxLen; ++l) {
    if (counts[l] >= lim - P) return fail(QM_E_UNSUPPORTED, "qm_gcb_expect: 2^63 fragments or more");
    P += counts[l];
    tab[2 * (size_t)l] = counts[l]; tab[2 * (size_t)l + 1] = ((1ULL << 31) + (u64)l - 1) / (u64)l;
  }
  if (g->maxTxpLen > 0 && P > (lim - 1) / (u64)g->maxTxpLen) return fail(QM_E_UNSUPPORTED, "qm_gcb_expect: fragments times the longest transcript reach 2^63");
  const qx::Stream st = g->stream;
  int rc;
  if (nTxps == 0) return QM_OK;
  if (g->nTiles < 0) {
    if ((rc = g->d_tileCnt.ensure(nTxps + 1)) || (rc = g->d_tileOff.ensure(nTxps + 1))) return rc;
    HIPCHK((qx::launch<gcb_tiles_wave>(st, qx::waves_of(nTxps + 1), g->I.txpLen, g->I.nTxp, g->d_tileCnt.p)));
    QXCHK(qx::scan_u32(st, g->d_tmp, g->d_tileCnt, g->d_tileOff, nTxps + 1));
    long long total = 0;
    QXCHK(qx::read(st, &total, g->d_tileOff + nTxps, sizeof(total)));
    g->nTiles = total;
  }
  if ((rc = g->d_tab.ensure((int64_t)tab.size())) || (rc = g->d_H.ensure(nTxps * GCB_BINS))) return rc;
  QXCHK(qx::upload(st, g->d_tab, tab.data(), tab.size() * sizeof(u64)));
  QXCHK(qx::fill(st, g->d_H, 0, (size_t)nTxps * GCB_BINS * sizeof(u64)));
  const GcbExp E{g->I.mask, g->I.txpOff, g->I.txpLen, g->d_tileOff, g->d_tab, g->d_H, g->I.nTxp, g->nTiles, g->maxLen};
  QXCHK(qx::tick(g->ev0, st));
  if (P && g->nTiles > 0) HIPCHK((qx::sweep<gcb_expect_wave>(st, sweep_grid(g->nTiles * 64, g->numCU, GCB_BLOCKS_PER_CU, g->maxBlocks), E)));
  QXCHK(qx::tick(g->ev1, st));
  QXCHK(qx::read(st, H, g->d_H, (size_t)nTxps * GCB_BINS * sizeof(u64)));   // (waits; the table on the host may go)
  qx::elapsed(g->ev0, g->ev1, &g->lastExpectUs);
  return QM_OK;
}

static int gcb_window_gc(qm_gcb* g, int64_t n, const uint32_t* tids, const int32_t* starts, const int32_t* lens, int32_t* out) {
  if (n <= 0) return QM_OK;
  const qx::Stream st = g->stream;
  int rc;
  if ((rc = g->d_qTid.ensure(n)) || (rc = g->d_qStart.ensure(n)) || (rc = g->d_qLen.ensure(n)) || (rc = g->d_qOut.ensure(n))) return rc;
  QXCHK(qx::upload(st, g->d_qTid, tids, (size_t)n * 4)); QXCHK(qx::upload(st, g->d_qStart, starts, (size_t)n * 4)); QXCHK(qx::upload(st, g->d_qLen, lens, (size_t)n * 4));
  HIPCHK((qx::launch<gcb_probe_wave>(st, qx::waves_of(n), g->I, (long long)n, (const u32*)g->d_qTid.p, (const int*)g->d_qStart.p, (const int*)g->d_qLen.p, g->d_qOut.p)));
  return qx::read(st, out, g->d_qOut, (size_t)n * 4);
}

#ifndef QM_EMU
// The replica's rank structure: built by the first qm_gcb of any context on that replica (under sanextMu, like the -s table)
static int ensure_gc_rank(qm_ctx* c, qm_gcb* g) {
  Replica& R = *c->rep;
  std::lock_guard<std::mutex> lk(R.sanextMu);
  if (!R.gcBuilt) {
    DevBuf<unsigned char> tmp;
    int rc = qx::tick(g->ev0, g->stream);
    if (!rc) rc = gcb_build_rank(g->stream, R.text, c->ix->n, R.gcMask, R.gcRank, tmp);
    if (!rc) rc = qx::tock(g->ev0, g->ev1, g->stream, &g->rankBuildUs);
    if (rc) { (void)hipGetLastError(); R.gcMask.release(); R.gcRank.release(); return fail(QM_E_NOGPU, "building the GC rank structure"); }
    R.gcBuilt = true;
    R.devBytes += gcb_blocks(c->ix->n) * 12;
  }
  c->devBytes = R.devBytes;
  g->I = GcbIdx{R.gcMask, R.gcRank, R.txpOff, R.txpLen, c->ix->nTxp, c->ix->n};
  return QM_OK;
}

extern "C" {

int qm_gcb_eff_lens_from_counts(int32_t max_len, const uint64_t* counts, int64_t n_txps, const uint32_t* lens, const uint64_t* H, const double* alpha,
                                const uint64_t* obs, double* eff, double* exp_out, double* ratio_out) {
#pragma clang fp contract(off)
  // S_t = sum of H[t][.] (integer); M_t = P[min(L_t, max_len)];
  // exp[b] = sum over t ascending with alpha_t > 0 and S_t > 0 of alpha_t * ((double)H[t][b] / (double)S_t): a division, a product, an addition
  // O = sum of obs (integer); E = sum over b ascending of exp[b]
  // ratio[b] = 1 when O == 0, E == 0 or exp[b] == 0; else min(max(((double)obs[b] / (double)O) / (exp[b] / E), 1e-3), 1e3)
  // e'_t = (double)L_t when M_t == 0; else (sum over b ascending of ratio[b] * (double)H[t][b]) / (double)M_t
  if (max_len < 1) return fail(QM_E_ARG, "qm_gcb_eff_lens: max_len %d", (int)max_len);
  if (max_len > GCB_MAX_LEN) return fail(QM_E_UNSUPPORTED, "qm_gcb_eff_lens: max_len %d beyond %d", (int)max_len, GCB_MAX_LEN);
  if (!counts || !obs || n_txps < 0 || (n_txps > 0 && (!lens || !H || !alpha || !eff))) return fail(QM_E_ARG, "qm_gcb_eff_lens: bad argument");
  if (counts[0]) return fail(QM_E_ARG, "qm_gcb_eff_lens: bin 0 holds %llu", (unsigned long long)counts[0]);
  std::vector<uint64_t> P((size_t)max_len + 1, 0);
  for (int l = 1; l <= max_len; ++l) {
    if (counts[l] >= (1ULL << 63) - P[(size_t)l - 1]) return fail(QM_E_UNSUPPORTED, "qm_gcb_eff_lens: 2^63 fragments or more");
    P[(size_t)l] = P[(size_t)l - 1] + counts[l];
  }
  double ex[GCB_BINS], ratio[GCB_BINS];
  for (int b = 0; b < GCB_BINS; ++b) ex[b] = 0.0;
  for (int64_t t = 0; t < n_txps; ++t) {
    if (!lens[t]) return fail(QM_E_ARG, "qm_gcb_eff_lens: transcript %lld has length 0", (long long)t);
    const uint64_t* h = H + (size_t)t * GCB_BINS;
    uint64_t S = 0;
    for (int b = 0; b < GCB_BINS; ++b) S += h[b];
    if (!(alpha[t] > 0.0) || !S) continue;
    for (int b = 0; b < GCB_BINS; ++b) { const double share = (double)h[b] / (double)S; const double w = alpha[t] * share; ex[b] = ex[b] + w; }
  }
  uint64_t O = 0; double E = 0.0;
  for (int b = 0; b < GCB_BINS; ++b) { O += obs[b]; E = E + ex[b]; }
  for (int b = 0; b < GCB_BINS; ++b) {
    if (!O || E == 0.0 || ex[b] == 0.0) { ratio[b] = 1.0; continue; }
    const double po = (double)obs[b] / (double)O, pe = ex[b] / E;
    double r = po / pe;
    if (r < 1e-3) r = 1e-3;
    if (r > 1e3) r = 1e3;
    ratio[b] = r;
  }
  for (int64_t t = 0; t < n_txps; ++t) {
    const uint64_t L = lens[t], M = P[(size_t)std::min<uint64_t>(L, (uint64_t)max_len)];
    if (!M) { eff[t] = (double)L; continue; }
    const uint64_t* h = H + (size_t)t * GCB_BINS;
    double s = 0.0;
    for (int b = 0; b < GCB_BINS; ++b) { const double w = ratio[b] * (double)h[b]; s = s + w; }
    eff[t] = s / (double)M;
  }
  for (int b = 0; b < GCB_BINS; ++b) { if (exp_out) exp_out[b] = ex[b]; if (ratio_out) ratio_out[b] = ratio[b]; }
  return QM_OK;
}

int qm_gcb_create(qm_ctx* c, int32_t max_len, uint32_t flags, qm_gcb** out) {
  if (!c || !out || (flags & ~0xffffu)) return fail(QM_E_ARG, "qm_gcb_create: bad argument");
  if (max_len < 1) return fail(QM_E_ARG, "qm_gcb_create: max_len %d", (int)max_len);
  if (max_len > GCB_MAX_LEN) return fail(QM_E_UNSUPPORTED, "qm_gcb_create: max_len %d beyond %d", (int)max_len, GCB_MAX_LEN);
  HIPCHK(hipSetDevice(c->device));
  qm_gcb* g = new qm_gcb();
  g->maxLen = max_len; g->maxBlocks = (int)(flags & 0xffffu);
  for (int64_t t = 0; t < c->ix->nTxp; ++t) g->maxTxpLen = std::max<long long>(g->maxTxpLen, (long long)c->ix->lens[(size_t)t]);
  int rc = g->open("qm_gcb_create", c->device, c->numCU);
  if (!rc && gcb_open(g) != QM_OK) rc = fail(QM_E_NOGPU, "qm_gcb_create: bins");
  if (!rc) rc = ensure_gc_rank(c, g);
  if (rc) { qm_gcb_destroy(g); return rc; }
  g->rep = c->rep;
  *out = g;
  return QM_OK;
}

int qm_gcb_destroy(qm_gcb* g) {
  if (!g) return QM_OK;
  g->close();
  delete g;                    // (the buffers free themselves; the replica lives while an object holds it)
  return QM_OK;
}

int qm_gcb_clear(qm_gcb* g) {
  QXCHK(qx::enter(g, true, "null object"));
  return gcb_clear(g);
}

int qm_gcb_add(qm_gcb* g, qm_ctx* c) {
  QXCHK(qx::enter_add(g, c, "qm_gcb_add", "GC counts", "fold"));
  if (c->rep.get() != g->rep.get()) return fail(QM_E_ARG, "qm_gcb_add: the context maps to another index");
  return gcb_fold(g, qx::last_units(c), c->stream);
}

int qm_gcb_add_hits(qm_gcb* g, int64_t n, const int64_t* offsets, const qm_hit* hits) {
  QXCHK(qx::enter(g, true, "qm_gcb_add_hits: bad argument"));
  return gcb_add_hits(g, n, offsets, hits, 1 << 22, 1 << 21);       // a part: what is uploaded and folded in one go
}

int qm_gcb_fetch(qm_gcb* g, uint64_t* obs) {
  QXCHK(qx::enter(g, obs != nullptr, "qm_gcb_fetch: bad argument"));
  return g->fetch(obs, GCB_BINS);
}

int qm_gcb_add_counts(qm_gcb* g, const uint64_t* obs) {
  QXCHK(qx::enter(g, obs != nullptr, "qm_gcb_add_counts: bad argument"));
  return gcb_add_counts(g, obs);
}

int qm_gcb_stat(const qm_gcb* g, int which, int64_t* value) {
  if (!g || !value) return fail(QM_E_ARG, "qm_gcb_stat: bad argument");
  return gcb_stat(g, which, value);
}

int qm_gcb_expect(qm_gcb* g, const uint64_t* counts, int64_t n_txps, uint64_t* H) {
  QXCHK(qx::enter(g, counts && n_txps >= 0 && (n_txps == 0 || H), "qm_gcb_expect: bad argument"));
  return gcb_expect(g, counts, n_txps, H);
}

int qm_gcb_window_gc(qm_gcb* g, int64_t n, const uint32_t* tids, const int32_t* starts, const int32_t* lens, int32_t* out) {
  QXCHK(qx::enter(g, n >= 0 && (n == 0 || (tids && starts && lens && out)), "qm_gcb_window_gc: bad argument"));
  return gcb_window_gc(g, n, tids, starts, lens, out);
}

}  // extern "C"
#endif
