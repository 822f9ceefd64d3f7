// qm_boot_host.inl -- host driver of the bootstrap replicates (device code: qm_boot.inl, kernels: qm_kernels_boot.hip).
// Included at the end of qm_host.hip, after qm_quant_host.inl: a qm_boot borrows the graph, the effective lengths and the stream
// of its qm_quant, and owns everything per replicate.
//
// create   = the snapshot's counts as integers, their exclusive scan (cum, N), and per side the queue of the rows of more than
//            BOOT_LONG items; the per-replicate arrays, replicate-innermost over Bp = n_reps rounded up to BOOT_TILE.
// resample = zero the counts, one launch of N / 2 Philox calls per slot, one launch for `single`, start values, bookkeeping.
// run      = per iteration a class launch and a transcript launch over rows / 4 x tiles; on a checking iteration a mark launch,
//            and the host reads ONE word (the replicates that are done); nothing otherwise.
// alpha is updated in place (the lane that writes alpha[t][rep] is the only one that reads it in that launch); the second alpha
// buffer holds the transposed copy [n_reps][n_txps] that qm_boot_fetch brings to the host in one piece.
#include "qm_boot.inl"

struct qm_boot {
  qm_quant* q = nullptr;
  int32_t nReps = 0; int64_t Bp = 0, nqCls = 0, nqTxp = 0;
  uint64_t N = 0; int64_t draws = 0;
  bool haveCounts = false, counted = false;                           // counted: the quant object knows of this one (qm_quant_destroy refuses while it lives)
  DevBuf<u64> d_cnt0, d_cum, d_cnt, d_col, d_rel, d_scal;
  DevBuf<double> d_single, d_w, d_r, d_alpha, d_alphaT, d_lastRel;
  DevBuf<u32> d_done; DevBuf<int> d_iters; DevBuf<long long> d_qCls, d_qTxp;
  DevBuf<unsigned char> d_tmp; PinBuf<u64> h_word;
  hipEvent_t ev0 = nullptr, ev1 = nullptr; int64_t lastResampleUs = 0, lastRunUs = 0, lastLaunches = 0;
  int aggregate = 0;                                                  // equal classes meet within a wavefront before the atomic (QM_BOOT_AGGREGATE=1)
};

static BootBook boot_book(qm_boot* b) { return BootBook{b->d_done, b->d_rel, b->d_iters, b->d_lastRel, b->d_scal}; }
static int boot_elapsed(qm_boot* b, int64_t* us) {
  HIPCHK(hipEventRecord(b->ev1, b->q->stream));
  HIPCHK(hipEventSynchronize(b->ev1));
  float ms = 0;
  if (hipEventElapsedTime(&ms, b->ev0, b->ev1) == hipSuccess) *us = (int64_t)(ms * 1000.0f + 0.5f);
  return QM_OK;
}
// one side's queue: the rows of more than BOOT_LONG items, ascending (flag, pos: n + 1 entries of scratch)
static int boot_side_queue(qm_boot* b, const long long* off, long long n, u32* flag, long long* pos, DevBuf<long long>& queue, int64_t* nq) {
  qm_quant* q = b->q; int rc; long long cnt = 0;
  HIPCHK(qmk_boot_rowflag(off, n, flag, q->stream));
  const size_t tb = qmk_quant_scan_temp_bytes(n + 1);
  if ((rc = b->d_tmp.ensure((int64_t)std::max<size_t>(tb, 1)))) return rc;
  HIPCHK(qmk_quant_scan(b->d_tmp, tb, flag, pos, n + 1, q->stream));
  if ((rc = quant_read(q, &cnt, pos + n, 8))) return rc;
  if ((rc = queue.ensure(std::max<int64_t>(cnt, 1)))) return rc;
  HIPCHK(qmk_quant_queue(flag, pos, n, queue, q->stream));
  *nq = cnt;
  return QM_OK;
}
// the snapshot's counts as 64-bit integers into dst[0 .. classes] (dst[classes] = 0)
static int boot_snapshot_counts(qm_quant* q, u64* dst) {
  if (q->total >> 53) return fail(QM_E_UNSUPPORTED, "the snapshot's counts add up to 2^53 or more: they are kept as doubles and no longer exact");
  HIPCHK(qmk_boot_counts(q->d_cnt, q->nClasses, (unsigned long long*)dst, q->stream));
  return QM_OK;
}

static int boot_build(qm_boot* b) {
  qm_quant* q = b->q; hipStream_t st = q->stream; int rc;
  const int64_t nc = q->nClasses, nT = q->nTxps, Bp = b->Bp;
  const int64_t perC = std::max<int64_t>(nc, 1) * Bp, perT = std::max<int64_t>(nT, 1) * Bp;
  if ((rc = b->d_cnt0.ensure(nc + 1)) || (rc = b->d_cum.ensure(nc + 1)) || (rc = b->d_col.ensure(nc + 1)) || (rc = b->d_cnt.ensure(perC)) || (rc = b->d_r.ensure(perC)) ||
      (rc = b->d_single.ensure(perT)) || (rc = b->d_w.ensure(perT)) || (rc = b->d_alpha.ensure(perT)) || (rc = b->d_alphaT.ensure(std::max<int64_t>(nT, 1) * b->nReps)) ||
      (rc = b->d_rel.ensure(Bp)) || (rc = b->d_lastRel.ensure(Bp)) || (rc = b->d_done.ensure(Bp)) || (rc = b->d_iters.ensure(Bp)) || (rc = b->d_scal.ensure(BOOT_SC_WORDS)) ||
      (rc = b->d_qCls.ensure(1)) || (rc = b->d_qTxp.ensure(1)) || (rc = b->h_word.ensure(1))) return rc;
  HIPCHK(hipMemsetAsync(b->d_cnt, 0, (size_t)perC * 8, st));
  HIPCHK(hipMemsetAsync(b->d_r, 0, (size_t)perC * 8, st));
  HIPCHK(hipMemsetAsync(b->d_single, 0, (size_t)perT * 8, st));
  HIPCHK(hipMemsetAsync(b->d_w, 0, (size_t)perT * 8, st));
  HIPCHK(hipMemsetAsync(b->d_alpha, 0, (size_t)perT * 8, st));
  HIPCHK(hipMemsetAsync(b->d_rel, 0, (size_t)Bp * 8, st));
  HIPCHK(hipMemsetAsync(b->d_iters, 0, (size_t)Bp * 4, st));
  HIPCHK(hipMemsetAsync(b->d_scal, 0, BOOT_SC_WORDS * 8, st));
  {
    std::vector<u32> done((size_t)Bp, 1u); std::vector<double> last((size_t)Bp, -1.0);     // the padding is done for good
    for (int32_t i = 0; i < b->nReps; ++i) done[(size_t)i] = 0;
    HIPCHK(hipMemcpyAsync(b->d_done, done.data(), (size_t)Bp * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(b->d_lastRel, last.data(), (size_t)Bp * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));                               // (the host vectors go away)
  }
  if ((rc = boot_snapshot_counts(q, b->d_cnt0))) return rc;
  {
    const size_t tb = qmk_boot_scan_temp_bytes(nc + 1);
    if ((rc = b->d_tmp.ensure((int64_t)std::max<size_t>(tb, 1)))) return rc;
    HIPCHK(qmk_boot_scan(b->d_tmp, tb, (const unsigned long long*)b->d_cnt0.p, (unsigned long long*)b->d_cum.p, nc + 1, st));
    if ((rc = quant_read(q, &b->N, b->d_cum + nc, 8))) return rc;
  }
  if (b->N != q->total) return fail(QM_E_STATE, "qm_boot_create: the snapshot's counts add up to %llu, the quant object has %llu", (unsigned long long)b->N, (unsigned long long)q->total);
  if (nc == 0) return QM_OK;
  DevBuf<u32> flag; DevBuf<long long> pos;
  const int64_t nflag = std::max(nc, nT) + 1;
  if ((rc = flag.ensure(nflag)) || (rc = pos.ensure(nflag))) return rc;
  if ((rc = boot_side_queue(b, q->d_coff, nc, flag, pos, b->d_qCls, &b->nqCls)) || (rc = boot_side_queue(b, q->d_toff, nT, flag, pos, b->d_qTxp, &b->nqTxp))) return rc;
  HIPCHK(hipStreamSynchronize(st));                                 // (flag and pos go away)
  return QM_OK;
}

// slots s0 .. s0 + ns - 1 have new counts adding up to `total`: single, start values and bookkeeping
static int boot_restart(qm_boot* b, int64_t s0, int64_t ns, uint64_t total) {
  qm_quant* q = b->q; hipStream_t st = q->stream;
  const double value = q->present > 0 ? (double)total / (double)q->present : 0.0;
  HIPCHK(qmk_boot_start(q->d_toff, q->d_eff, q->nTxps, value, b->d_alpha, b->d_w, b->Bp, s0, ns, st));
  BootBook K = boot_book(b);
  HIPCHK(qmk_boot_reset(&K, s0, ns, st));
  return QM_OK;
}

extern "C" {

int qm_quant_fetch_classes(qm_quant* q, int64_t* offsets, uint32_t* tids, uint64_t* counts) {
  if (!q || !offsets || (q->nEntries > 0 && !tids) || (q->nClasses > 0 && !counts)) return fail(QM_E_ARG, "qm_quant_fetch_classes: bad argument");
  HIPCHK(hipSetDevice(q->device));
  int rc;
  DevBuf<u64> c64;
  if ((rc = c64.ensure(q->nClasses + 1)) || (rc = boot_snapshot_counts(q, c64))) return rc;
  if ((rc = quant_read(q, offsets, q->d_coff, (size_t)(q->nClasses + 1) * 8))) return rc;
  if (q->nEntries > 0 && (rc = quant_read(q, tids, q->d_clab, (size_t)q->nEntries * 4))) return rc;
  if (q->nClasses > 0 && (rc = quant_read(q, counts, c64, (size_t)q->nClasses * 8))) return rc;
  return QM_OK;
}

int qm_boot_create(qm_quant* q, int32_t n_reps, qm_boot** out) {
  if (!q || !out || n_reps < 1) return fail(QM_E_ARG, "qm_boot_create: bad argument");
  if (n_reps > 65535) return fail(QM_E_UNSUPPORTED, "qm_boot_create: more than 65535 replicates in one object (run them in batches: first_rep)");
  HIPCHK(hipSetDevice(q->device));
  qm_boot* b = new qm_boot();
  b->q = q; b->nReps = n_reps; b->Bp = boot_padded(n_reps);
  const char* ag = getenv("QM_BOOT_AGGREGATE");
  if (ag && *ag) b->aggregate = atoi(ag) != 0;
  int rc = QM_OK;
  if (hipEventCreate(&b->ev0) != hipSuccess || hipEventCreate(&b->ev1) != hipSuccess) rc = fail(QM_E_NOGPU, "qm_boot_create: events");
  if (!rc) rc = boot_build(b);
  if (rc) { qm_boot_destroy(b); return rc; }
  q->boots++; b->counted = true;
  *out = b;
  return QM_OK;
}

int qm_boot_destroy(qm_boot* b) {
  if (!b) return QM_OK;
  hipSetDevice(b->q->device);
  hipStreamSynchronize(b->q->stream);
  if (b->ev0) hipEventDestroy(b->ev0);
  if (b->ev1) hipEventDestroy(b->ev1);
  if (b->counted) b->q->boots--;
  delete b;                    // (the buffers free themselves)
  return QM_OK;
}

int qm_boot_resample(qm_boot* b, uint64_t seed, int64_t first_rep) {
  if (!b) return fail(QM_E_ARG, "null boot object");
  qm_quant* q = b->q; hipStream_t st = q->stream; int rc;
  HIPCHK(hipSetDevice(q->device));
  HIPCHK(hipEventRecord(b->ev0, st));
  if (q->nClasses > 0) {
    HIPCHK(hipMemsetAsync(b->d_cnt, 0, (size_t)q->nClasses * b->Bp * 8, st));
    BootDraw D{b->d_cum, q->nClasses, b->N, seed, (u64)first_rep, b->d_cnt, b->Bp, b->aggregate};
    HIPCHK(qmk_boot_resample(&D, b->nReps, b->aggregate, st));
    HIPCHK(qmk_boot_single(q->d_coff, q->d_clab, q->nClasses, (const unsigned long long*)b->d_cnt.p, b->d_single, b->Bp, st));
  }
  if ((rc = boot_restart(b, 0, b->nReps, b->N))) return rc;
  b->draws = (int64_t)b->N; b->haveCounts = true;
  return boot_elapsed(b, &b->lastResampleUs);
}

int qm_boot_set_counts(qm_boot* b, int32_t rep, const uint64_t* counts) {
  if (!b || rep < 0 || rep >= b->nReps || (b->q->nClasses > 0 && !counts)) return fail(QM_E_ARG, "qm_boot_set_counts: bad argument");
  qm_quant* q = b->q; hipStream_t st = q->stream; int rc;
  HIPCHK(hipSetDevice(q->device));
  uint64_t total = 0;
  for (int64_t c = 0; c < q->nClasses; ++c) total += counts[c];
  if (q->nClasses > 0) {
    HIPCHK(hipMemcpyAsync(b->d_col, counts, (size_t)q->nClasses * 8, hipMemcpyHostToDevice, st));
    HIPCHK(qmk_boot_column(q->d_coff, q->d_clab, q->nClasses, (unsigned long long*)b->d_cnt.p, b->d_single, b->Bp, rep, (unsigned long long*)b->d_col.p, 1, st));
  }
  if ((rc = boot_restart(b, rep, 1, total))) return rc;
  HIPCHK(hipStreamSynchronize(st));                                 // (the caller's array is free again)
  b->haveCounts = true;
  return QM_OK;
}

int qm_boot_fetch_counts(qm_boot* b, int32_t rep, uint64_t* counts) {
  if (!b || rep < 0 || rep >= b->nReps || (b->q->nClasses > 0 && !counts)) return fail(QM_E_ARG, "qm_boot_fetch_counts: bad argument");
  qm_quant* q = b->q;
  HIPCHK(hipSetDevice(q->device));
  if (q->nClasses == 0) return QM_OK;
  HIPCHK(qmk_boot_column(q->d_coff, q->d_clab, q->nClasses, (unsigned long long*)b->d_cnt.p, b->d_single, b->Bp, rep, (unsigned long long*)b->d_col.p, 0, q->stream));
  return quant_read(q, counts, b->d_col, (size_t)q->nClasses * 8);
}

int qm_boot_run(qm_boot* b, int32_t max_iter, int32_t check_every, double rel_tol, double min_alpha, int32_t* iterations, double* last_rel_change) {
  if (!b || max_iter < 0 || check_every < 1 || !(rel_tol >= 0) || !(min_alpha >= 0)) return fail(QM_E_ARG, "qm_boot_run: bad argument");
  if (!b->haveCounts) return fail(QM_E_STATE, "qm_boot_run: no counts yet (qm_boot_resample or qm_boot_set_counts first)");
  qm_quant* q = b->q; hipStream_t st = q->stream; int rc;
  HIPCHK(hipSetDevice(q->device));
  BootBook K = boot_book(b);
  int32_t it = 0; int64_t launches = 0;
  HIPCHK(hipEventRecord(b->ev0, st));
  HIPCHK(qmk_boot_begin(&K, b->nReps, st));
  if ((rc = quant_read(q, b->h_word.p, b->d_scal + BOOT_SC_DONE, 8))) return rc;   // (before the first launch: is anything still running?)
  if (q->nClasses > 0 && max_iter > 0 && *b->h_word.p < (u64)b->nReps) {
    BootState S{};
    S.cls = QuantCsr{q->d_coff, q->d_clab, q->nClasses, b->d_qCls, b->nqCls};
    S.txp = QuantCsr{q->d_toff, q->d_tcls, q->nTxps, b->d_qTxp, b->nqTxp};
    S.eff = q->d_eff; S.cnt = b->d_cnt; S.single = b->d_single; S.w = b->d_w; S.r = b->d_r; S.alpha = b->d_alpha; S.rel = b->d_rel; S.done = b->d_done;
    S.Bp = b->Bp; S.minAlpha = min_alpha;
    while (it < max_iter) {
      const bool check = rel_tol > 0 && (it + 1) % check_every == 0;
      S.check = check ? 1 : 0;
      HIPCHK(qmk_boot_class(&S, st));
      HIPCHK(qmk_boot_txp(&S, st));
      ++it; launches += 2;
      if (check) {                                                  // the one word the host reads
        HIPCHK(qmk_boot_mark(&K, b->nReps, it, rel_tol, st)); ++launches;
        if ((rc = quant_read(q, b->h_word.p, b->d_scal + BOOT_SC_DONE, 8))) return rc;
        if (*b->h_word.p >= (u64)b->nReps) break;
      }
    }
  }
  HIPCHK(qmk_boot_end(&K, b->nReps, it, st));
  if (iterations && (rc = quant_read(q, iterations, b->d_iters, (size_t)b->nReps * 4))) return rc;
  if (last_rel_change && (rc = quant_read(q, last_rel_change, b->d_lastRel, (size_t)b->nReps * 8))) return rc;
  b->lastLaunches = launches;
  return boot_elapsed(b, &b->lastRunUs);
}

int qm_boot_fetch(qm_boot* b, double* alpha) {
  if (!b || (b->q->nTxps > 0 && !alpha)) return fail(QM_E_ARG, "qm_boot_fetch: bad argument");
  qm_quant* q = b->q;
  HIPCHK(hipSetDevice(q->device));
  if (q->nTxps == 0) return QM_OK;
  HIPCHK(qmk_boot_transpose(b->d_alpha, q->nTxps, b->Bp, b->nReps, b->d_alphaT, q->stream));
  return quant_read(q, alpha, b->d_alphaT, (size_t)q->nTxps * b->nReps * 8);
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
