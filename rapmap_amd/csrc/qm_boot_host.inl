// qm_boot_host.inl -- host driver of the bootstrap replicates (device code: qm_boot.inl).
// Included at the end of qm_host.hip, after qm_quant_host.inl: a qm_boot borrows the graph, the effective lengths and the stream
// of its qm_quant, and owns everything per replicate.
// Everything above the extern "C" block is written against qm_exec.h and compiled twice: here, and with -DQM_EMU by tests/emu.
//
// open     = the snapshot's counts as integers, their exclusive scan (cum, N), and per side the queue of the rows of more than
//            BOOT_LONG items; the per-replicate arrays, replicate-innermost over Bp = n_reps rounded up to BOOT_TILE.
// resample = zero the counts, one launch of N / 2 Philox calls per slot, one launch for `single`, start values, bookkeeping.
// run      = per iteration a class launch and a transcript launch over rows / 4 x tiles; on a checking iteration a mark launch,
//            and the host reads ONE word (the replicates that are done); nothing otherwise.
// alpha is updated in place (the lane that writes alpha[t][rep] is the only one that reads it in that launch); the second alpha
// buffer holds the transposed copy [n_reps][n_txps] that qm_boot_fetch brings to the host in one piece.
#include "qm_boot.inl"
#include "qm_exec.h"

struct qm_boot : qx::Base {      // (opened on its quant's stream: it owns the two events only)
  qm_quant* q = nullptr;
  int32_t nReps = 0; int64_t Bp = 0, nqCls = 0, nqTxp = 0;
  uint64_t N = 0; int64_t draws = 0;
  bool haveCounts = false, counted = false;                           // counted: the quant object knows of this one (qm_quant_destroy refuses while it lives)
  DevBuf<u64> d_cnt0, d_cum, d_cnt, d_col, d_rel, d_scal;
  DevBuf<double> d_single, d_w, d_r, d_alpha, d_alphaT, d_lastRel;
  DevBuf<u32> d_done; DevBuf<int> d_iters; DevBuf<long long> d_qCls, d_qTxp;
  DevBuf<unsigned char> d_tmp; PinBuf<u64> h_word;
  int64_t lastResampleUs = 0, lastRunUs = 0, lastLaunches = 0;
  int aggregate = 0;                                                  // equal classes meet within a wavefront before the atomic (QM_BOOT_AGGREGATE=1)
};

static BootBook boot_book(qm_boot* b) { return BootBook{b->d_done, b->d_rel, b->d_iters, b->d_lastRel, b->d_scal}; }
// (the aggregation is decided when the kernel is compiled)
template <int AGG>
QM_DEV void boot_resample_body(BootDraw D, long long wave, long long slot) { D.aggregate = AGG; boot_resample_wave(D, wave, slot); }

// one side's queue: the rows of more than BOOT_LONG items, ascending (flag, pos: n + 1 entries of scratch)
static int boot_side_queue(qm_boot* b, const long long* off, long long n, u32* flag, long long* pos, DevBuf<long long>& queue, int64_t* nq) {
  qm_quant* q = b->q; int rc; long long cnt = 0;
  HIPCHK(qx::launch<boot_rowflag_wave>(q->stream, qx::waves_of(n + 1), off, n, flag));
  if ((rc = qx::scan_u32(q->stream, b->d_tmp, flag, pos, n + 1)) || (rc = qx::read(q->stream, &cnt, pos + n, 8))) return rc;
  if ((rc = queue.ensure(std::max<int64_t>(cnt, 1)))) return rc;
  HIPCHK(qx::launch<quant_queue_wave>(q->stream, qx::waves_of(n), (const u32*)flag, (const long long*)pos, n, queue.p));
  *nq = cnt;
  return QM_OK;
}
// the snapshot's counts as 64-bit integers into dst[0 .. classes] (dst[classes] = 0)
static int boot_snapshot_counts(qm_quant* q, u64* dst) {
  if (q->total >> 53) return fail(QM_E_UNSUPPORTED, "the snapshot's counts add up to 2^53 or more: they are kept as doubles and no longer exact");
  HIPCHK(qx::launch<boot_counts_wave>(q->stream, qx::waves_of(q->nClasses + 1), (const double*)q->d_cnt.p, (long long)q->nClasses, dst));
  return QM_OK;
}
static int quant_fetch_classes(qm_quant* q, int64_t* offsets, uint32_t* tids, uint64_t* counts) {
  int rc;
  DevBuf<u64> c64;
  if ((rc = c64.ensure(q->nClasses + 1)) || (rc = boot_snapshot_counts(q, c64))) return rc;
  if ((rc = qx::read(q->stream, offsets, q->d_coff, (size_t)(q->nClasses + 1) * 8))) return rc;
  if (q->nEntries > 0 && (rc = qx::read(q->stream, tids, q->d_clab, (size_t)q->nEntries * 4))) return rc;
  if (q->nClasses > 0 && (rc = qx::read(q->stream, counts, c64, (size_t)q->nClasses * 8))) return rc;
  return QM_OK;
}

static int boot_build(qm_boot* b) {
  qm_quant* q = b->q; qx::Stream st = q->stream; int rc;
  const int64_t nc = q->nClasses, nT = q->nTxps, Bp = b->Bp;
  const int64_t perC = std::max<int64_t>(nc, 1) * Bp, perT = std::max<int64_t>(nT, 1) * Bp;
  if ((rc = b->d_cnt0.ensure(nc + 1)) || (rc = b->d_cum.ensure(nc + 1)) || (rc = b->d_col.ensure(nc + 1)) || (rc = b->d_cnt.ensure(perC)) || (rc = b->d_r.ensure(perC)) ||
      (rc = b->d_single.ensure(perT)) || (rc = b->d_w.ensure(perT)) || (rc = b->d_alpha.ensure(perT)) || (rc = b->d_alphaT.ensure(std::max<int64_t>(nT, 1) * b->nReps)) ||
      (rc = b->d_rel.ensure(Bp)) || (rc = b->d_lastRel.ensure(Bp)) || (rc = b->d_done.ensure(Bp)) || (rc = b->d_iters.ensure(Bp)) || (rc = b->d_scal.ensure(BOOT_SC_WORDS)) ||
      (rc = b->d_qCls.ensure(1)) || (rc = b->d_qTxp.ensure(1)) || (rc = b->h_word.ensure(1))) return rc;
  QXCHK(qx::fill(st, b->d_cnt, 0, (size_t)perC * 8));
  QXCHK(qx::fill(st, b->d_r, 0, (size_t)perC * 8));
  QXCHK(qx::fill(st, b->d_single, 0, (size_t)perT * 8));
  QXCHK(qx::fill(st, b->d_w, 0, (size_t)perT * 8));
  QXCHK(qx::fill(st, b->d_alpha, 0, (size_t)perT * 8));
  QXCHK(qx::fill(st, b->d_rel, 0, (size_t)Bp * 8));
  QXCHK(qx::fill(st, b->d_iters, 0, (size_t)Bp * 4));
  QXCHK(qx::fill(st, b->d_scal, 0, BOOT_SC_WORDS * 8));
  {
    std::vector<u32> done((size_t)Bp, 1u); std::vector<double> last((size_t)Bp, -1.0);     // the padding is done for good
    for (int32_t i = 0; i < b->nReps; ++i) done[(size_t)i] = 0;
    QXCHK(qx::upload(st, b->d_done, done.data(), (size_t)Bp * 4));
    QXCHK(qx::upload(st, b->d_lastRel, last.data(), (size_t)Bp * 8));
    QXCHK(qx::sync(st));                                            // (the host vectors go away)
  }
  if ((rc = boot_snapshot_counts(q, b->d_cnt0)) || (rc = qx::scan_u64(st, b->d_tmp, b->d_cnt0, b->d_cum, nc + 1)) || (rc = qx::read(st, &b->N, b->d_cum + nc, 8))) return rc;
  if (b->N != q->total) return fail(QM_E_STATE, "qm_boot_create: the snapshot's counts add up to %llu, the quant object has %llu", (unsigned long long)b->N, (unsigned long long)q->total);
  if (nc == 0) return QM_OK;
  DevBuf<u32> flag; DevBuf<long long> pos;
  const int64_t nflag = std::max(nc, nT) + 1;
  if ((rc = flag.ensure(nflag)) || (rc = pos.ensure(nflag))) return rc;
  if ((rc = boot_side_queue(b, q->d_coff, nc, flag, pos, b->d_qCls, &b->nqCls)) || (rc = boot_side_queue(b, q->d_toff, nT, flag, pos, b->d_qTxp, &b->nqTxp))) return rc;
  return qx::sync(st);                                              // (flag and pos go away)
}
// a new object (its events are there) on q: everything per replicate; q counts it from here on
static int boot_open(qm_boot* b, qm_quant* q, int32_t n_reps) {
  if (n_reps < 1) return fail(QM_E_ARG, "qm_boot_create: bad argument");
  if (n_reps > 65535) return fail(QM_E_UNSUPPORTED, "qm_boot_create: more than 65535 replicates in one object (run them in batches: first_rep)");
  b->q = q; b->nReps = n_reps; b->Bp = boot_padded(n_reps);
  if (int rc = boot_build(b)) return rc;
  q->boots++; b->counted = true;
  return QM_OK;
}
static void boot_close(qm_boot* b) { if (b->counted) b->q->boots--; b->counted = false; }

// slots s0 .. s0 + ns - 1 have new counts adding up to `total`: single, start values and bookkeeping
static int boot_restart(qm_boot* b, int64_t s0, int64_t ns, uint64_t total) {
  qm_quant* q = b->q; qx::Stream st = q->stream;
  const double value = q->present > 0 ? (double)total / (double)q->present : 0.0;
  // (the method and the prior are the quant object's, and fixed while this object lives: qm_quant_set_method refuses)
  if (q->method == QM_QUANT_METHOD_VBEM)
    HIPCHK(qx::launch2<boot_start_vb_wave>(st, boot_row_waves(q->nTxps), b->Bp / BOOT_TILE, (const long long*)q->d_toff.p, (const double*)q->d_eff.p, (const double*)q->d_prior.p,
                                           (long long)q->nTxps, value, b->d_alpha.p, b->d_w.p, (long long)b->Bp, (long long)s0, (long long)ns));
  else
    HIPCHK(qx::launch2<boot_start_wave>(st, boot_row_waves(q->nTxps), b->Bp / BOOT_TILE, (const long long*)q->d_toff.p, (const double*)q->d_eff.p, (long long)q->nTxps, value,
                                        b->d_alpha.p, b->d_w.p, (long long)b->Bp, (long long)s0, (long long)ns));
  HIPCHK(qx::launch<boot_reset_wave>(st, qx::waves_of(ns), boot_book(b), (long long)s0, (long long)ns));
  return QM_OK;
}

static int boot_resample(qm_boot* b, uint64_t seed, int64_t first_rep) {
  qm_quant* q = b->q; qx::Stream st = q->stream; int rc;
  QXCHK(qx::tick(b->ev0, st));
  if (q->nClasses > 0) {
    QXCHK(qx::fill(st, b->d_cnt, 0, (size_t)q->nClasses * b->Bp * 8));
    const BootDraw D{b->d_cum, q->nClasses, b->N, seed, (u64)first_rep, b->d_cnt, b->Bp, b->aggregate};
    const long long waves = (long long)(((b->N + 1) / 2 + 63) / 64);   // (N + 1) / 2 Philox calls per slot
    if (b->aggregate) HIPCHK(qx::launch2<boot_resample_body<1>>(st, waves, b->nReps, D));
    else HIPCHK(qx::launch2<boot_resample_body<0>>(st, waves, b->nReps, D));
    HIPCHK(qx::launch2<boot_single_wave>(st, boot_row_waves(q->nClasses), b->Bp / BOOT_TILE, (const long long*)q->d_coff.p, (const u32*)q->d_clab.p, (long long)q->nClasses,
                                         (const u64*)b->d_cnt.p, b->d_single.p, (long long)b->Bp));
  }
  if ((rc = boot_restart(b, 0, b->nReps, b->N))) return rc;
  b->draws = (int64_t)b->N; b->haveCounts = true;
  return qx::tock(b->ev0, b->ev1, st, &b->lastResampleUs);
}

// one slot's counts to (put = 0) or from (put = 1) d_col
static int boot_column(qm_boot* b, int32_t rep, int put) {
  qm_quant* q = b->q;
  HIPCHK(qx::launch<boot_column_wave>(q->stream, qx::waves_of(q->nClasses), (const long long*)q->d_coff.p, (const u32*)q->d_clab.p, (long long)q->nClasses, b->d_cnt.p, b->d_single.p,
                                      (long long)b->Bp, (long long)rep, b->d_col.p, put));
  return QM_OK;
}
static int boot_set_counts(qm_boot* b, int32_t rep, const uint64_t* counts) {
  if (rep < 0 || rep >= b->nReps) return fail(QM_E_ARG, "qm_boot_set_counts: bad argument");
  qm_quant* q = b->q; qx::Stream st = q->stream; int rc;
  uint64_t total = 0;
  for (int64_t c = 0; c < q->nClasses; ++c) total += counts[c];
  if (q->nClasses > 0) {
    QXCHK(qx::upload(st, b->d_col, counts, (size_t)q->nClasses * 8));
    if ((rc = boot_column(b, rep, 1))) return rc;
  }
  if ((rc = boot_restart(b, rep, 1, total)) || (rc = qx::sync(st))) return rc;   // (the caller's array is free again)
  b->haveCounts = true;
  return QM_OK;
}
static int boot_fetch_counts(qm_boot* b, int32_t rep, uint64_t* counts) {
  if (rep < 0 || rep >= b->nReps) return fail(QM_E_ARG, "qm_boot_fetch_counts: bad argument");
  qm_quant* q = b->q; int rc;
  if (q->nClasses == 0) return QM_OK;
  if ((rc = boot_column(b, rep, 0))) return rc;
  return qx::read(q->stream, counts, b->d_col, (size_t)q->nClasses * 8);
}

static int boot_run(qm_boot* b, int32_t max_iter, int32_t check_every, double rel_tol, double min_alpha, int32_t* iterations, double* last_rel_change) {
  if (max_iter < 0 || check_every < 1 || !(rel_tol >= 0) || !(min_alpha >= 0)) return fail(QM_E_ARG, "qm_boot_run: bad argument");
  if (!b->haveCounts) return fail(QM_E_STATE, "qm_boot_run: no counts yet (qm_boot_resample or qm_boot_set_counts first)");
  qm_quant* q = b->q; qx::Stream st = q->stream; int rc;
  const BootBook K = boot_book(b);
  const long long nReps = b->nReps, tiles = b->Bp / BOOT_TILE;
  int32_t it = 0; int64_t launches = 0;
  QXCHK(qx::tick(b->ev0, st));
  HIPCHK(qx::launch<boot_begin_wave>(st, qx::waves_of(nReps), K, nReps));
  if ((rc = qx::read(st, b->h_word.p, b->d_scal + BOOT_SC_DONE, 8))) return rc;   // (before the first launch: is anything still running?)
  if (q->nClasses > 0 && max_iter > 0 && *b->h_word.p < (u64)b->nReps) {
    BootState S{};
    S.cls = QuantCsr{q->d_coff, q->d_clab, q->nClasses, b->d_qCls, b->nqCls};
    S.txp = QuantCsr{q->d_toff, q->d_tcls, q->nTxps, b->d_qTxp, b->nqTxp};
    S.eff = q->d_eff; S.cnt = b->d_cnt; S.single = b->d_single; S.w = b->d_w; S.r = b->d_r; S.alpha = b->d_alpha; S.rel = b->d_rel; S.done = b->d_done;
    S.Bp = b->Bp; S.minAlpha = min_alpha;
    while (it < max_iter) {
      const bool check = rel_tol > 0 && (it + 1) % check_every == 0;
      S.check = check ? 1 : 0;
      HIPCHK(qx::launch2<boot_class_wave>(st, boot_side_waves(S.cls), tiles, S));
      if (q->method == QM_QUANT_METHOD_VBEM) HIPCHK(qx::launch2<boot_txp_vb_wave>(st, boot_side_waves(S.txp), tiles, S, (const double*)q->d_prior.p));
      else HIPCHK(qx::launch2<boot_txp_wave>(st, boot_side_waves(S.txp), tiles, S));
      ++it; launches += 2;
      if (check) {                                                  // the one word the host reads
        HIPCHK(qx::launch<boot_mark_wave>(st, qx::waves_of(nReps), K, nReps, (int)it, rel_tol)); ++launches;
        if ((rc = qx::read(st, b->h_word.p, b->d_scal + BOOT_SC_DONE, 8))) return rc;
        if (*b->h_word.p >= (u64)b->nReps) break;
      }
    }
  }
  HIPCHK(qx::launch<boot_end_wave>(st, qx::waves_of(nReps), K, nReps, (int)it));
  if (iterations && (rc = qx::read(st, iterations, b->d_iters, (size_t)b->nReps * 4))) return rc;
  if (last_rel_change && (rc = qx::read(st, last_rel_change, b->d_lastRel, (size_t)b->nReps * 8))) return rc;
  b->lastLaunches = launches;
  return qx::tock(b->ev0, b->ev1, st, &b->lastRunUs);
}

static int boot_fetch(qm_boot* b, double* alpha) {
  qm_quant* q = b->q;
  if (q->nTxps == 0) return QM_OK;
  HIPCHK(qx::launch2<boot_transpose_wave>(q->stream, qx::waves_of(q->nTxps), b->nReps, (const double*)b->d_alpha.p, (long long)q->nTxps, (long long)b->Bp, b->d_alphaT.p));
  return qx::read(q->stream, alpha, b->d_alphaT, (size_t)q->nTxps * b->nReps * 8);
}

#ifndef QM_EMU
extern "C" {

int qm_quant_fetch_classes(qm_quant* q, int64_t* offsets, uint32_t* tids, uint64_t* counts) {
  if (!q || !offsets || (q->nEntries > 0 && !tids) || (q->nClasses > 0 && !counts)) return fail(QM_E_ARG, "qm_quant_fetch_classes: bad argument");
  HIPCHK(hipSetDevice(q->device));
  return quant_fetch_classes(q, offsets, tids, counts);
}

int qm_boot_create(qm_quant* q, int32_t n_reps, qm_boot** out) {
  if (!q || !out) return fail(QM_E_ARG, "qm_boot_create: bad argument");
  HIPCHK(hipSetDevice(q->device));
  qm_boot* b = new qm_boot();
  b->q = q;
  const char* ag = getenv("QM_BOOT_AGGREGATE");
  if (ag && *ag) b->aggregate = atoi(ag) != 0;
  int rc = b->open("qm_boot_create", q->device, q->numCU, &q->stream);     // the quant's stream, borrowed
  if (!rc) rc = boot_open(b, q, n_reps);
  if (rc) { qm_boot_destroy(b); return rc; }
  *out = b;
  return QM_OK;
}

int qm_boot_destroy(qm_boot* b) {
  if (!b) return QM_OK;
  b->close();                  // (waits for the borrowed stream and leaves it to the quant object)
  boot_close(b);
  delete b;                    // (the buffers free themselves)
  return QM_OK;
}

int qm_boot_resample(qm_boot* b, uint64_t seed, int64_t first_rep) {
  if (!b) return fail(QM_E_ARG, "null boot object");
  HIPCHK(hipSetDevice(b->q->device));
  return boot_resample(b, seed, first_rep);
}

int qm_boot_set_counts(qm_boot* b, int32_t rep, const uint64_t* counts) {
  if (!b || (b->q->nClasses > 0 && !counts)) return fail(QM_E_ARG, "qm_boot_set_counts: bad argument");
  HIPCHK(hipSetDevice(b->q->device));
  return boot_set_counts(b, rep, counts);
}

int qm_boot_fetch_counts(qm_boot* b, int32_t rep, uint64_t* counts) {
  if (!b || (b->q->nClasses > 0 && !counts)) return fail(QM_E_ARG, "qm_boot_fetch_counts: bad argument");
  HIPCHK(hipSetDevice(b->q->device));
  return boot_fetch_counts(b, rep, counts);
}

int qm_boot_run(qm_boot* b, int32_t max_iter, int32_t check_every, double rel_tol, double min_alpha, int32_t* iterations, double* last_rel_change) {
  if (!b) return fail(QM_E_ARG, "qm_boot_run: bad argument");
  HIPCHK(hipSetDevice(b->q->device));
  return boot_run(b, max_iter, check_every, rel_tol, min_alpha, iterations, last_rel_change);
}

int qm_boot_fetch(qm_boot* b, double* alpha) {
  if (!b || (b->q->nTxps > 0 && !alpha)) return fail(QM_E_ARG, "qm_boot_fetch: bad argument");
  HIPCHK(hipSetDevice(b->q->device));
  return boot_fetch(b, alpha);
}

int qm_boot_stat(const qm_boot* b, int which, int64_t* value) {
  if (!b || !value) return fail(QM_E_ARG, "qm_boot_stat: bad argument");
  switch (which) {
    case QM_BOOT_STAT_REPLICATES: *value = b->nReps; break;
    case QM_BOOT_STAT_DRAWS: *value = b->draws; break;
    case QM_BOOT_STAT_LAST_RESAMPLE_US: *value = b->lastResampleUs; break;
    case QM_BOOT_STAT_LAST_RUN_US: *value = b->lastRunUs; break;
    case QM_BOOT_STAT_LAUNCHES: *value = b->lastLaunches; break;
    case QM_BOOT_STAT_QUEUED_LABELS: *value = b->nqCls; break;
    case QM_BOOT_STAT_QUEUED_TXPS: *value = b->nqTxp; break;
    default: return fail(QM_E_ARG, "qm_boot_stat: unknown statistic %d", which);
  }
  return QM_OK;
}

}  // extern "C"
#endif
