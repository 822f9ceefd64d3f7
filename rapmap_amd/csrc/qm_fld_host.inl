// qm_fld_host.inl -- host driver of the fragment-length histogram (device code: qm_fld.inl, kernel: qm_kernels_fld.hip) and the
// arithmetic from histogram to effective lengths.  Included at the end of qm_host.hip: qm_fld_add reads the context's last result
// where it lies in device memory.
//
// A fold = one launch of a persistent grid, then the six counters (and nothing else) read back.  The effective lengths are host
// arithmetic over the fetched bins: once per run over 8 KB, off the per-batch path.
#include <algorithm>
#include "qm_fld.inl"

struct qm_fld {
  int device = 0, numCU = 256, maxLen = QM_FLD_DEFAULT_MAX_LEN, maxBlocks = 0;
  hipStream_t stream = nullptr;
  DevBuf<u64> d_acc;                                                  // FLD_ACC_WORDS: the bins, then the counters
  u64 h[FLD_C_WORDS] = {0};                                           // the counters as last read
  DevBuf<long long> d_inOff; DevBuf<qm_hit> d_inHits;                 // qm_fld_add_hits
  int64_t units = 0, folds = 0, lastFoldUs = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;                            // around the last fold's kernel on its stream
};

static int fld_fold(qm_fld* f, const FldSrc& S, hipStream_t st) {
  if (S.n <= 0) return QM_OK;
  if (S.n >= (1LL << 32)) return fail(QM_E_ARG, "more than 2^32 - 1 units in one fold");   // (a wavefront's 32-bit bins cannot overflow)
  const FldAcc A{f->d_acc, f->d_acc + FLD_SLAB, f->maxLen};
  HIPCHK(hipEventRecord(f->ev0, st));
  HIPCHK(qmk_fld_fold(&S, &A, qmk_fld_grid(S.n, f->numCU, f->maxBlocks), st));
  HIPCHK(hipEventRecord(f->ev1, st));
  HIPCHK(hipMemcpyAsync(f->h, f->d_acc + FLD_SLAB, sizeof(f->h), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  float ms = 0;
  if (hipEventElapsedTime(&ms, f->ev0, f->ev1) == hipSuccess) f->lastFoldUs = (int64_t)(ms * 1000.0f + 0.5f);
  f->units += S.n; f->folds++;
  return QM_OK;
}

extern "C" {

int qm_fld_eff_lens_from_counts(int32_t max_len, const uint64_t* counts, int64_t n_txps, const uint32_t* lens, double* eff) {
#pragma clang fp contract(off)
  if (max_len < 1) return fail(QM_E_ARG, "qm_fld_eff_lens: max_len %d", (int)max_len);
  if (max_len > FLD_SLAB - 1) return fail(QM_E_UNSUPPORTED, "qm_fld_eff_lens: max_len %d beyond %d", (int)max_len, FLD_SLAB - 1);
  if (!counts || n_txps < 0 || (n_txps > 0 && (!lens || !eff))) return fail(QM_E_ARG, "qm_fld_eff_lens: bad argument");
  if (counts[0]) return fail(QM_E_ARG, "qm_fld_eff_lens: bin 0 holds %llu", (unsigned long long)counts[0]);
  const uint64_t lim = 1ULL << 53;
  std::vector<uint64_t> P((size_t)max_len + 1, 0), Q((size_t)max_len + 1, 0);
  for (int l = 1; l <= max_len; ++l) {
    if (counts[l] > lim / (uint64_t)l) return fail(QM_E_UNSUPPORTED, "qm_fld_eff_lens: the fragment lengths add up to 2^53 or more");
    P[(size_t)l] = P[(size_t)l - 1] + counts[l]; Q[(size_t)l] = Q[(size_t)l - 1] + (uint64_t)l * counts[l];
    if (Q[(size_t)l] >= lim) return fail(QM_E_UNSUPPORTED, "qm_fld_eff_lens: the fragment lengths add up to 2^53 or more");
  }
  for (int64_t t = 0; t < n_txps; ++t) {
    const uint64_t L = lens[t];
    if (!L) return fail(QM_E_ARG, "qm_fld_eff_lens: transcript %lld has length 0", (long long)t);
    const size_t m = (size_t)std::min<uint64_t>(L, (uint64_t)max_len);
    if (!P[m]) { eff[t] = (double)L; continue; }
    const double mean = (double)Q[m] / (double)P[m];
    eff[t] = (double)(L + 1) - mean;
  }
  return QM_OK;
}

int qm_fld_create(qm_ctx* c, int32_t max_len, uint32_t flags, qm_fld** out) {
  if (!c || !out || (flags & ~0xffffu)) return fail(QM_E_ARG, "qm_fld_create: bad argument");
  if (max_len < 1) return fail(QM_E_ARG, "qm_fld_create: max_len %d", (int)max_len);
  if (max_len > FLD_SLAB - 1) return fail(QM_E_UNSUPPORTED, "qm_fld_create: max_len %d beyond %d", (int)max_len, FLD_SLAB - 1);
  HIPCHK(hipSetDevice(c->device));
  qm_fld* f = new qm_fld();
  f->device = c->device; f->numCU = c->numCU; f->maxLen = max_len; f->maxBlocks = (int)(flags & 0xffffu);
  int rc = QM_OK;
  if (hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking) != hipSuccess || f->d_acc.ensure(FLD_ACC_WORDS) != QM_OK) rc = fail(QM_E_NOGPU, "qm_fld_create: stream / bins");
  if (!rc && (hipEventCreate(&f->ev0) != hipSuccess || hipEventCreate(&f->ev1) != hipSuccess)) rc = fail(QM_E_NOGPU, "qm_fld_create: events");
  if (!rc && (hipMemsetAsync(f->d_acc, 0, FLD_ACC_WORDS * sizeof(u64), f->stream) != hipSuccess || hipStreamSynchronize(f->stream) != hipSuccess)) rc = fail(QM_E_NOGPU, "qm_fld_create: memset");
  if (rc) { qm_fld_destroy(f); return rc; }
  *out = f;
  return QM_OK;
}

int qm_fld_destroy(qm_fld* f) {
  if (!f) return QM_OK;
  hipSetDevice(f->device);
  if (f->stream) hipStreamSynchronize(f->stream);
  if (f->ev0) hipEventDestroy(f->ev0);
  if (f->ev1) hipEventDestroy(f->ev1);
  if (f->stream) hipStreamDestroy(f->stream);
  delete f;                    // (the buffers free themselves)
  return QM_OK;
}

int qm_fld_clear(qm_fld* f) {
  if (!f) return fail(QM_E_ARG, "null histogram");
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(hipMemsetAsync(f->d_acc, 0, FLD_ACC_WORDS * sizeof(u64), f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  memset(f->h, 0, sizeof(f->h));
  f->units = f->folds = f->lastFoldUs = 0;
  return QM_OK;
}

int qm_fld_add(qm_fld* f, qm_ctx* c) {
  if (!f || !c) return fail(QM_E_ARG, "qm_fld_add: null argument");
  if (c->last.units < 0) return fail(QM_E_STATE, "no mapping result to fold");
  if (c->device != f->device) return fail(QM_E_ARG, "histogram on device %d, context on device %d", f->device, c->device);
  HIPCHK(hipSetDevice(f->device));
  const FldSrc S{(const unsigned char*)c->d_hits.p, (int)sizeof(qm_hit), c->d_offs, c->last.units};
  return fld_fold(f, S, c->stream);
}

int qm_fld_add_hits(qm_fld* f, int64_t n, const int64_t* offsets, const qm_hit* hits) {
  if (!f || n < 0 || (n > 0 && !offsets)) return fail(QM_E_ARG, "qm_fld_add_hits: bad argument");
  for (int64_t i = 0; i < n; ++i) if (offsets[i + 1] < offsets[i]) return fail(QM_E_ARG, "qm_fld_add_hits: offsets decrease at unit %lld", (long long)i);
  if (n > 0 && offsets[n] > offsets[0] && !hits) return fail(QM_E_ARG, "qm_fld_add_hits: null hits");
  HIPCHK(hipSetDevice(f->device));
  const int64_t maxUnits = 1 << 22, maxHits = 1 << 21;           // a part: what is uploaded and folded in one go
  std::vector<long long> off;
  int rc;
  for (int64_t u0 = 0; u0 < n;) {
    int64_t u1 = u0 + 1;
    while (u1 < n && u1 - u0 < maxUnits && offsets[u1 + 1] - offsets[u0] <= maxHits) ++u1;
    const int64_t nu = u1 - u0, nh = offsets[u1] - offsets[u0];
    off.resize((size_t)nu + 1);
    for (int64_t i = 0; i <= nu; ++i) off[(size_t)i] = offsets[u0 + i] - offsets[u0];
    if ((rc = f->d_inOff.ensure(nu + 1)) || (nh > 0 && (rc = f->d_inHits.ensure(nh)))) return rc;
    HIPCHK(hipMemcpyAsync(f->d_inOff, off.data(), (size_t)(nu + 1) * 8, hipMemcpyHostToDevice, f->stream));
    if (nh > 0) HIPCHK(hipMemcpyAsync(f->d_inHits, hits + offsets[u0], (size_t)nh * sizeof(qm_hit), hipMemcpyHostToDevice, f->stream));
    HIPCHK(hipStreamSynchronize(f->stream));                    // (the host vector is reused)
    const FldSrc S{nh > 0 ? (const unsigned char*)f->d_inHits.p : nullptr, (int)sizeof(qm_hit), f->d_inOff, nu};
    if ((rc = fld_fold(f, S, f->stream))) return rc;
    u0 = u1;
  }
  return QM_OK;
}

int qm_fld_fetch(qm_fld* f, uint64_t* counts) {
  if (!f || !counts) return fail(QM_E_ARG, "qm_fld_fetch: bad argument");
  HIPCHK(hipSetDevice(f->device));
  HIPCHK(hipMemcpyAsync(counts, f->d_acc, (size_t)(f->maxLen + 1) * sizeof(u64), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  return QM_OK;
}

int qm_fld_add_counts(qm_fld* f, const uint64_t* counts) {
  if (!f || !counts) return fail(QM_E_ARG, "qm_fld_add_counts: bad argument");
  if (counts[0]) return fail(QM_E_ARG, "qm_fld_add_counts: bin 0 holds %llu", (unsigned long long)counts[0]);
  HIPCHK(hipSetDevice(f->device));
  // off the per-batch path: the bins and the `used` counter come to the host, are added to and go back
  std::vector<u64> acc(FLD_ACC_WORDS);
  HIPCHK(hipMemcpyAsync(acc.data(), f->d_acc, FLD_ACC_WORDS * sizeof(u64), hipMemcpyDeviceToHost, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  u64 sum = 0;
  for (int l = 1; l <= f->maxLen; ++l) { acc[(size_t)l] += counts[l]; sum += counts[l]; }
  acc[FLD_SLAB + FLD_C_USED] += sum;
  HIPCHK(hipMemcpyAsync(f->d_acc, acc.data(), FLD_ACC_WORDS * sizeof(u64), hipMemcpyHostToDevice, f->stream));
  HIPCHK(hipStreamSynchronize(f->stream));
  memcpy(f->h, acc.data() + FLD_SLAB, sizeof(f->h));
  f->units += (int64_t)sum;
  return QM_OK;
}

int qm_fld_stat(const qm_fld* f, int which, int64_t* value) {
  if (!f || !value) return fail(QM_E_ARG, "qm_fld_stat: bad argument");
  switch (which) {
    case QM_FLD_STAT_UNITS: *value = f->units; break;
    case QM_FLD_STAT_USED: *value = (int64_t)f->h[FLD_C_USED]; break;
    case QM_FLD_STAT_UNMAPPED: *value = (int64_t)f->h[FLD_C_UNMAPPED]; break;
    case QM_FLD_STAT_MULTI: *value = (int64_t)f->h[FLD_C_MULTI]; break;
    case QM_FLD_STAT_NOT_PAIRED: *value = (int64_t)f->h[FLD_C_NOT_PAIRED]; break;
    case QM_FLD_STAT_SAME_STRAND: *value = (int64_t)f->h[FLD_C_SAME_STRAND]; break;
    case QM_FLD_STAT_OUT_OF_RANGE: *value = (int64_t)f->h[FLD_C_OUT_OF_RANGE]; break;
    case QM_FLD_STAT_MAX_LEN: *value = f->maxLen; break;
    case QM_FLD_STAT_FOLDS: *value = f->folds; break;
    case QM_FLD_STAT_LAST_FOLD_US: *value = f->lastFoldUs; break;
    default: return fail(QM_E_ARG, "qm_fld_stat: unknown statistic %d", which);
  }
  return QM_OK;
}

int qm_fld_eff_lens(qm_fld* f, int64_t n_txps, const uint32_t* lens, double* eff) {
  if (!f) return fail(QM_E_ARG, "qm_fld_eff_lens: null histogram");
  std::vector<uint64_t> counts((size_t)f->maxLen + 1);
  const int rc = qm_fld_fetch(f, counts.data());
  return rc ? rc : qm_fld_eff_lens_from_counts(f->maxLen, counts.data(), n_txps, lens, eff);
}

}  // extern "C"
