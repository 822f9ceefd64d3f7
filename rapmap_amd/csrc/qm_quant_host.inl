// qm_quant_host.inl -- host driver of the EM over an equivalence-class table (device code: qm_quant.inl).
// Included at the end of qm_host.hip, after qm_eqc_host.inl: the structure build reads a qm_eqc where it lies in device memory.
// Everything above the extern "C" block is written against qm_exec.h and compiled twice: here, and with -DQM_EMU by tests/emu.
//
// open = the structure build: mark / two scans / compact (a snapshot of the published slots as a class-side CSR, in ascending
// slot order), a stable sort of the (tid, class) pairs and a bounds launch (the transcript side, classes ascending), then per side
// row statistics, a scan and the queue of the rows of more than QNT_GROUP items.  The quant object owns everything it made and its
// own stream; the table may be folded into, cleared or destroyed afterwards.
// run = per iteration a class launch and a transcript launch on that stream; the host reads ONE word on a checking iteration
// (every check_every-th), nothing otherwise.  The method (EM or variational Bayes) and the prior are state of the object: a run
// begins with the weights of the current alpha under its method and launches that method's transcript kernel.
#include <cmath>
#include "qm_quant.inl"
#include "qm_exec.h"

struct qm_quant : qx::Base {
  int64_t nTxps = 0, nClasses = 0, nEntries = 0, present = 0, maxLabel = 0, maxList = 0, nqCls = 0, nqTxp = 0;
  uint64_t total = 0;                                                 // the sum of the snapshot's counts
  DevBuf<long long> d_coff, d_toff, d_qCls, d_qTxp; DevBuf<u32> d_clab, d_tcls;
  DevBuf<double> d_cnt, d_eff, d_single, d_w, d_r, d_alpha[2]; int cur = 0;     // alpha: two buffers, d_alpha[cur] holds the current one
  DevBuf<u64> d_scal; u64 h[QNT_SC_WORDS] = {0}; PinBuf<u64> h_rel;
  DevBuf<unsigned char> d_tmp;                                        // the scans' and the sort's scratch (structure build)
  int method = QM_QUANT_METHOD_EM; DevBuf<double> d_prior;           // the weight of a transcript (quant_weight); the prior: [n_txps], made by the first set_method
  int boots = 0;                                                      // live qm_boot objects that borrow the graph and the stream (qm_boot_host.inl)
  int64_t lastRunUs = 0, buildUs = 0;                                 // the events: around the last run / the structure build on its stream (QM_QUANT_STAT_LAST_RUN_US, _BUILD_US)
};

// one side's queue: the rows of more than QNT_GROUP items, ascending (flag, pos: n + 1 entries of scratch)
static int quant_side_queue(qm_quant* q, const long long* off, long long n, u32* flag, long long* pos, int maxWord, int present, DevBuf<long long>& queue, int64_t* nq) {
  int rc; long long cnt = 0;
  HIPCHK(qx::launch<quant_rowstat_wave>(q->stream, qx::waves_of(n + 1), off, n, flag, q->d_scal.p, maxWord, present));
  if ((rc = qx::scan_u32(q->stream, q->d_tmp, flag, pos, n + 1)) || (rc = qx::read(q->stream, &cnt, pos + n, 8))) return rc;
  if ((rc = queue.ensure(std::max<int64_t>(cnt, 1)))) return rc;
  HIPCHK(qx::launch<quant_queue_wave>(q->stream, qx::waves_of(n), (const u32*)flag, (const long long*)pos, n, queue.p));
  *nq = cnt;
  return QM_OK;
}

static int quant_build(qm_quant* q, qm_eqc* t, const double* eff) {
  qx::Stream st = q->stream; int rc;
  int64_t nc0 = 0, ne0 = 0; uint64_t total = 0;
  if ((rc = eqc_size(t, &nc0, &ne0, &total))) return rc;             // (ends with a read-back on the table's stream: the table is at rest)
  q->total = total;
  const long long cap = (long long)(t->T.mask + 1), nT = q->nTxps;
  const long long nflag = std::max(cap, nT) + 1;
  DevBuf<u32> flag, len, pairTid, pairCls, sortedTid; DevBuf<long long> cidx, lofs;
  if ((rc = flag.ensure(nflag)) || (rc = len.ensure(cap + 1)) || (rc = cidx.ensure(nflag)) || (rc = lofs.ensure(cap + 1))) return rc;
  QXCHK(qx::fill(st, q->d_scal, 0, sizeof(q->h)));
  QuantBuild B{};
  B.key = t->T.key; B.llen = t->T.llen; B.loff = t->T.loff; B.count = t->T.count; B.pool = t->T.pool; B.cap = cap;
  B.flag = flag; B.len = len; B.cidx = cidx; B.lofs = lofs; B.nTxps = (u64)nT; B.scal = q->d_scal;
  HIPCHK(qx::launch<quant_mark_wave>(st, qx::waves_of(cap + 1), B));
  if ((rc = qx::scan_u32(st, q->d_tmp, flag, cidx, cap + 1)) || (rc = qx::scan_u32(st, q->d_tmp, len, lofs, cap + 1))) return rc;
  long long nc = 0, ne = 0;
  if ((rc = qx::read(st, &nc, cidx + cap, 8)) || (rc = qx::read(st, &ne, lofs + cap, 8))) return rc;
  if (nc != nc0 || ne != ne0) return fail(QM_E_STATE, "qm_quant_create: %lld published slots with %lld tids, the table counts %lld and %lld", nc, ne, (long long)nc0, (long long)ne0);
  if (ne >= (1LL << 31)) return fail(QM_E_UNSUPPORTED, "qm_quant_create: more than 2^31 - 1 label entries");
  q->nClasses = nc; q->nEntries = ne;
  const int64_t nT1 = std::max<int64_t>(nT, 1);
  if ((rc = q->d_alpha[0].ensure(nT1)) || (rc = q->d_alpha[1].ensure(nT1)) || (rc = q->d_w.ensure(nT1)) ||
      (rc = q->d_eff.ensure(nT1)) || (rc = q->d_single.ensure(nT1)) || (rc = q->d_toff.ensure(nT + 1)) || (rc = q->d_r.ensure(std::max<int64_t>(nc, 1))) ||
      (rc = q->d_cnt.ensure(std::max<int64_t>(nc, 1))) || (rc = q->d_coff.ensure(nc + 1)) || (rc = q->d_clab.ensure(std::max<int64_t>(ne, 1))) ||
      (rc = q->d_tcls.ensure(std::max<int64_t>(ne, 1))) || (rc = q->d_qCls.ensure(1)) || (rc = q->d_qTxp.ensure(1))) return rc;
  {
    std::vector<double> e((size_t)nT, 1.0);
    if (eff) memcpy(e.data(), eff, (size_t)nT * 8);
    if (nT > 0) QXCHK(qx::upload(st, q->d_eff, e.data(), (size_t)nT * 8));
    QXCHK(qx::sync(st));                                            // (the host vector goes away)
  }
  QXCHK(qx::fill(st, q->d_alpha[0], 0, (size_t)nT1 * 8));
  QXCHK(qx::fill(st, q->d_alpha[1], 0, (size_t)nT1 * 8));
  QXCHK(qx::fill(st, q->d_w, 0, (size_t)nT1 * 8));
  QXCHK(qx::fill(st, q->d_single, 0, (size_t)nT1 * 8));
  QXCHK(qx::fill(st, q->d_toff, 0, (size_t)(nT + 1) * 8));
  QXCHK(qx::fill(st, q->d_coff, 0, (size_t)(nc + 1) * 8));
  if (nc == 0) return qx::sync(st);                                 // an empty table: nothing to iterate over
  if ((rc = pairTid.ensure(ne)) || (rc = pairCls.ensure(ne)) || (rc = sortedTid.ensure(ne))) return rc;
  B.coff = q->d_coff; B.clab = q->d_clab; B.cnt = q->d_cnt; B.pairTid = pairTid; B.pairCls = pairCls; B.single = q->d_single;
  HIPCHK(qx::launch<quant_compact_wave>(st, qx::waves_of(cap + 1), B));
  if ((rc = qx::read(st, q->h, q->d_scal, sizeof(q->h)))) return rc;
  if (q->h[QNT_SC_BAD_TID]) return fail(QM_E_ARG, "qm_quant_create: %llu label entries name a transcript beyond n_txps = %lld", (unsigned long long)q->h[QNT_SC_BAD_TID], nT);
  if ((rc = qx::sort_pairs(st, q->d_tmp, pairTid, sortedTid, pairCls, q->d_tcls, ne))) return rc;
  HIPCHK(qx::launch<quant_bounds_wave>(st, qx::waves_of(nT + 1), (const u32*)sortedTid.p, ne, nT, q->d_toff.p));
  if ((rc = quant_side_queue(q, q->d_coff, nc, flag, cidx, QNT_SC_MAX_LABEL, 0, q->d_qCls, &q->nqCls)) ||
      (rc = quant_side_queue(q, q->d_toff, nT, flag, cidx, QNT_SC_MAX_LIST, 1, q->d_qTxp, &q->nqTxp)) ||
      (rc = qx::read(st, q->h, q->d_scal, sizeof(q->h)))) return rc;
  q->present = (int64_t)q->h[QNT_SC_PRESENT]; q->maxLabel = (int64_t)q->h[QNT_SC_MAX_LABEL]; q->maxList = (int64_t)q->h[QNT_SC_MAX_LIST];
  return QM_OK;
}

static int quant_set_start(qm_quant* q, const double* alpha0) {
  if (alpha0) for (int64_t i = 0; i < q->nTxps; ++i) if (!(alpha0[i] >= 0) || !std::isfinite(alpha0[i])) return fail(QM_E_ARG, "qm_quant_set_start: alpha0[%lld] is not a non-negative finite number", (long long)i);
  if (q->nTxps == 0) return QM_OK;
  double* a = q->d_alpha[q->cur];
  if (alpha0) QXCHK(qx::upload(q->stream, a, alpha0, (size_t)q->nTxps * 8));
  else if (q->present == 0) QXCHK(qx::fill(q->stream, a, 0, (size_t)q->nTxps * 8));
  else HIPCHK(qx::launch<quant_start_wave>(q->stream, qx::waves_of(q->nTxps), (const long long*)q->d_toff.p, (long long)q->nTxps, (double)q->total / (double)q->present, a));
  return qx::sync(q->stream);
}

// what qm_quant_create checks of its values (before anything is made)
static int quant_check(int64_t n_txps, const double* eff) {
  if (n_txps < 0 || n_txps > 0xffffffffLL) return fail(QM_E_ARG, "qm_quant_create: bad argument");
  if (eff) for (int64_t i = 0; i < n_txps; ++i) if (!(eff[i] > 0) || !std::isfinite(eff[i])) return fail(QM_E_ARG, "qm_quant_create: effective length %lld is not a positive finite number", (long long)i);
  return QM_OK;
}
// a new object (stream and events are there): the scalars, the structure build, the uniform start
static int quant_open(qm_quant* q, qm_eqc* t, int64_t n_txps, const double* eff) {
  int rc;
  q->nTxps = n_txps;
  if ((rc = q->d_scal.ensure(QNT_SC_WORDS)) || (rc = q->h_rel.ensure(1)) || (rc = qx::tick(q->ev0, q->stream)) || (rc = quant_build(q, t, eff)) ||
      (rc = qx::tock(q->ev0, q->ev1, q->stream, &q->buildUs))) return rc;
  return quant_set_start(q, nullptr);
}
static int quant_may_close(const qm_quant* q) {
  return q->boots > 0 ? fail(QM_E_STATE, "qm_quant_destroy: %d bootstrap object(s) still borrow this quant object", q->boots) : QM_OK;
}

// the method of every later run, and of the replicates of a qm_boot made later; alpha stays as it is (a run begins with the weights
// of the current alpha under its method)
static int quant_set_method(qm_quant* q, int method, const double* prior) {
  if (method != QM_QUANT_METHOD_EM && method != QM_QUANT_METHOD_VBEM) return fail(QM_E_ARG, "qm_quant_set_method: unknown method %d", method);
  if (method == QM_QUANT_METHOD_VBEM && prior) for (int64_t i = 0; i < q->nTxps; ++i) if (!(prior[i] >= 0) || !std::isfinite(prior[i])) return fail(QM_E_ARG, "qm_quant_set_method: prior[%lld] is not a non-negative finite number", (long long)i);
  if (q->boots > 0) return fail(QM_E_STATE, "qm_quant_set_method: %d bootstrap object(s) borrow this quant object", q->boots);
  if (method == QM_QUANT_METHOD_VBEM) {
    const int64_t nT1 = std::max<int64_t>(q->nTxps, 1); int rc;
    if ((rc = q->d_prior.ensure(nT1))) return rc;
    if (prior && q->nTxps > 0) QXCHK(qx::upload(q->stream, q->d_prior, prior, (size_t)q->nTxps * 8));
    else QXCHK(qx::fill(q->stream, q->d_prior, 0, (size_t)nT1 * 8));
    QXCHK(qx::sync(q->stream));                                     // (the caller's array is free again)
  }
  q->method = method;
  return QM_OK;
}

// E over an array (qm_quant.inl: quant_exp_digamma): one launch on `st`
static int quant_exp_digamma_array(qx::Stream st, const double* x, int64_t n, double* out) {
  if (n < 0 || (n > 0 && (!x || !out))) return fail(QM_E_ARG, "qm_quant_exp_digamma: bad argument");
  if (n == 0) return QM_OK;
  DevBuf<double> dx, dy; int rc;
  if ((rc = dx.ensure(n)) || (rc = dy.ensure(n))) return rc;
  QXCHK(qx::upload(st, dx, x, (size_t)n * 8));
  HIPCHK(qx::launch<quant_exp_digamma_wave>(st, qx::waves_of(n), (const double*)dx.p, (long long)n, dy.p));
  return qx::read(st, out, dy, (size_t)n * 8);
}

static int quant_run(qm_quant* q, int32_t max_iter, int32_t check_every, double rel_tol, double min_alpha, int32_t* iterations, double* last_rel_change) {
  if (max_iter < 0 || check_every < 1 || !(rel_tol >= 0) || !(min_alpha >= 0)) return fail(QM_E_ARG, "qm_quant_run: bad argument");
  qx::Stream st = q->stream;
  const bool vb = q->method == QM_QUANT_METHOD_VBEM;
  const double* prior = q->d_prior.p;
  int32_t it = 0; double rel = -1.0; int rc;
  QXCHK(qx::tick(q->ev0, st));
  if (q->nClasses > 0 && max_iter > 0) {
    if (vb) HIPCHK(qx::launch<quant_weights_vb_wave>(st, qx::waves_of(q->nTxps), (const double*)q->d_alpha[q->cur].p, (const double*)q->d_eff.p, prior, (long long)q->nTxps, q->d_w.p));
    else HIPCHK(qx::launch<quant_weights_wave>(st, qx::waves_of(q->nTxps), (const double*)q->d_alpha[q->cur].p, (const double*)q->d_eff.p, (long long)q->nTxps, q->d_w.p));
    QuantState Q{};
    Q.cls = QuantCsr{q->d_coff, q->d_clab, q->nClasses, q->d_qCls, q->nqCls};
    Q.txp = QuantCsr{q->d_toff, q->d_tcls, q->nTxps, q->d_qTxp, q->nqTxp};
    Q.cnt = q->d_cnt; Q.eff = q->d_eff; Q.single = q->d_single; Q.w = q->d_w; Q.r = q->d_r; Q.scal = q->d_scal; Q.minAlpha = min_alpha;
    while (it < max_iter) {
      const bool check = rel_tol > 0 && (it + 1) % check_every == 0;
      Q.alpha = q->d_alpha[q->cur]; Q.alphaNew = q->d_alpha[q->cur ^ 1]; Q.check = check ? 1 : 0;
      if (check) QXCHK(qx::fill(st, q->d_scal + QNT_SC_REL, 0, sizeof(u64)));
      HIPCHK(qx::launch<quant_class_wave>(st, quant_side_waves(Q.cls), Q));
      if (vb) HIPCHK(qx::launch<quant_txp_vb_wave>(st, quant_side_waves(Q.txp), Q, prior));
      else HIPCHK(qx::launch<quant_txp_wave>(st, quant_side_waves(Q.txp), Q));
      q->cur ^= 1; ++it;
      if (check) {                                                  // the one word the host reads
        if ((rc = qx::read(st, q->h_rel.p, q->d_scal + QNT_SC_REL, sizeof(u64)))) return rc;
        memcpy(&rel, q->h_rel.p, 8);
        if (rel < rel_tol) break;
      }
    }
  }
  if ((rc = qx::tock(q->ev0, q->ev1, st, &q->lastRunUs))) return rc;
  if (iterations) *iterations = it;
  if (last_rel_change) *last_rel_change = rel;
  return QM_OK;
}

static int quant_fetch(qm_quant* q, double* alpha) {
  return q->nTxps == 0 ? QM_OK : qx::read(q->stream, alpha, q->d_alpha[q->cur], (size_t)q->nTxps * 8);
}

#ifndef QM_EMU
extern "C" {

int qm_quant_create(qm_eqc* t, int64_t n_txps, const double* eff_len, qm_quant** out) {
  if (!t || !out) return fail(QM_E_ARG, "qm_quant_create: bad argument");
  int rc;
  if ((rc = quant_check(n_txps, eff_len))) return rc;
  HIPCHK(hipSetDevice(t->device));
  qm_quant* q = new qm_quant();
  rc = q->open("qm_quant_create", t->device, t->numCU);
  if (!rc) rc = quant_open(q, t, n_txps, eff_len);
  if (rc) { qm_quant_destroy(q); return rc; }
  *out = q;
  return QM_OK;
}

int qm_quant_destroy(qm_quant* q) {
  if (!q) return QM_OK;
  if (int rc = quant_may_close(q)) return rc;
  q->close();
  delete q;                    // (the buffers free themselves)
  return QM_OK;
}

int qm_quant_set_start(qm_quant* q, const double* alpha0) {
  if (!q) return fail(QM_E_ARG, "null quant object");
  HIPCHK(hipSetDevice(q->device));
  return quant_set_start(q, alpha0);
}

int qm_quant_set_method(qm_quant* q, int method, const double* prior) {
  if (!q) return fail(QM_E_ARG, "null quant object");
  HIPCHK(hipSetDevice(q->device));
  return quant_set_method(q, method, prior);
}

int qm_quant_exp_digamma(int device, const double* x, int64_t n, double* out) {
  HIPCHK(hipSetDevice(device));
  return quant_exp_digamma_array(nullptr, x, n, out);              // (the null stream: no object is at hand)
}

int qm_quant_run(qm_quant* q, int32_t max_iter, int32_t check_every, double rel_tol, double min_alpha, int32_t* iterations, double* last_rel_change) {
  if (!q) return fail(QM_E_ARG, "qm_quant_run: bad argument");
  HIPCHK(hipSetDevice(q->device));
  return quant_run(q, max_iter, check_every, rel_tol, min_alpha, iterations, last_rel_change);
}

int qm_quant_fetch(qm_quant* q, double* alpha) {
  if (!q || (q->nTxps > 0 && !alpha)) return fail(QM_E_ARG, "qm_quant_fetch: bad argument");
  HIPCHK(hipSetDevice(q->device));
  return quant_fetch(q, alpha);
}

int qm_quant_stat(const qm_quant* q, int which, int64_t* value) {
  if (!q || !value) return fail(QM_E_ARG, "qm_quant_stat: bad argument");
  switch (which) {
    case QM_QUANT_STAT_CLASSES: *value = q->nClasses; break;
    case QM_QUANT_STAT_ENTRIES: *value = q->nEntries; break;
    case QM_QUANT_STAT_PRESENT: *value = q->present; break;
    case QM_QUANT_STAT_LONGEST_LABEL: *value = q->maxLabel; break;
    case QM_QUANT_STAT_LONGEST_LIST: *value = q->maxList; break;
    case QM_QUANT_STAT_QUEUED_LABELS: *value = q->nqCls; break;
    case QM_QUANT_STAT_QUEUED_TXPS: *value = q->nqTxp; break;
    case QM_QUANT_STAT_LAST_RUN_US: *value = q->lastRunUs; break;
    case QM_QUANT_STAT_BUILD_US: *value = q->buildUs; break;
    default: return fail(QM_E_ARG, "qm_quant_stat: unknown statistic %d", which);
  }
  return QM_OK;
}

}  // extern "C"
#endif
