// qm_fld_host.inl -- host driver of the fragment-length histogram (device code: qm_fld.inl, kernel: qm_kernels_fld.hip) and the
// arithmetic from histogram to effective lengths.  Included at the end of qm_host.hip: qm_fld_add reads the context's last result
// where it lies in device memory.  Everything above the extern "C" block is written against qm_exec.h and compiled twice: here, and
// with -DQM_EMU by tests/emu.
//
// A fold = one launch of a persistent grid, then the six counters (and nothing else) read back: one host wait.  The effective
// lengths are host arithmetic over the fetched bins: once per run over 8 KB, off the per-batch path.
#include <algorithm>
#include "qm_fld.inl"
#include "qm_exec.h"
#include "qm_grid.h"

struct qm_fld : qx::Base {
  int maxLen = QM_FLD_DEFAULT_MAX_LEN, maxBlocks = 0;
  DevBuf<u64> d_acc;                                                  // FLD_ACC_WORDS: the bins, then the counters
  u64 h[FLD_C_WORDS] = {0};                                           // the counters as last read
  qx::FeedBuf in;                                                     // qm_fld_add_hits
  int64_t units = 0, folds = 0, lastFoldUs = 0;                       // (the events: around the last fold's kernel on its stream)
};

// the kernel (qm_kernels_fld.hip, declared in qm_device.h) as the emulation runs it: four wavefronts per workgroup, one after the
// other, each on a slab filled with 0xA5 -- the body must zero what it uses
#ifdef QM_EMU
static int qmk_fld_fold(const FldSrc& S, const FldAcc& A, int blocks, qx::Stream) {
  if (S.n <= 0 || blocks <= 0) return 0;
  std::vector<u32> slab(FLD_SLAB);
  for (long long w = 0; w < 4LL * blocks; ++w) {
    slab.assign(FLD_SLAB, 0xA5A5A5A5u);
    fld_wave(S, A, w, 4LL * blocks, slab.data());
  }
  return 0;
}
#endif

static int fld_clear(qm_fld* f) {
  int rc;
  if ((rc = qx::fill(f->stream, f->d_acc, 0, FLD_ACC_WORDS * sizeof(u64))) || (rc = qx::sync(f->stream))) return rc;
  memset(f->h, 0, sizeof(f->h));
  f->units = f->folds = f->lastFoldUs = 0;
  return QM_OK;
}
static int fld_open(qm_fld* f) {
  const int rc = f->d_acc.ensure(FLD_ACC_WORDS);
  return rc ? rc : fld_clear(f);
}

static int fld_fold(qm_fld* f, const FldSrc& S, qx::Stream st) {
  if (S.n <= 0) return QM_OK;
  if (S.n >= (1LL << 32)) return fail(QM_E_ARG, "more than 2^32 - 1 units in one fold");   // (a wavefront's 32-bit bins cannot overflow)
  const FldAcc A{f->d_acc, f->d_acc + FLD_SLAB, f->maxLen};
  QXCHK(qx::tick(f->ev0, st));
  HIPCHK(qmk_fld_fold(S, A, sweep_grid(S.n, f->numCU, FLD_BLOCKS_PER_CU, f->maxBlocks), st));
  QXCHK(qx::tick(f->ev1, st));
  QXCHK(qx::read(st, f->h, f->d_acc + FLD_SLAB, sizeof(f->h)));       // (the one wait of a fold: both events have passed)
  qx::elapsed(f->ev0, f->ev1, &f->lastFoldUs);
  f->units += S.n; f->folds++;
  return QM_OK;
}

// qm_fld_add_hits: the host arrays in parts (at most maxUnits units and maxHits hits each) through the fold
static int fld_add_hits(qm_fld* f, int64_t n, const int64_t* offsets, const qm_hit* hits, int64_t maxUnits, int64_t maxHits) {
  return qx::feed(f->stream, f->in, "qm_fld_add_hits", "unit", "hits", n, offsets, hits, sizeof(qm_hit), nullptr, maxUnits, maxHits,
                  [&](const long long* off, const unsigned char* h, const u64*, int64_t, int64_t nu, int64_t) {
                    return fld_fold(f, FldSrc{h, (int)sizeof(qm_hit), off, nu}, f->stream);
                  });
}

static int fld_fetch(qm_fld* f, uint64_t* counts) { return qx::read(f->stream, counts, f->d_acc, (size_t)(f->maxLen + 1) * sizeof(u64)); }

static int fld_add_counts(qm_fld* f, const uint64_t* counts) {
  if (counts[0]) return fail(QM_E_ARG, "qm_fld_add_counts: bin 0 holds %llu", (unsigned long long)counts[0]);
  // off the per-batch path: the bins and the `used` counter come to the host, are added to and go back
  std::vector<u64> acc(FLD_ACC_WORDS);
  QXCHK(qx::read(f->stream, acc.data(), f->d_acc, FLD_ACC_WORDS * sizeof(u64)));
  u64 sum = 0;
  for (int l = 1; l <= f->maxLen; ++l) { acc[(size_t)l] += counts[l]; sum += counts[l]; }
  acc[FLD_SLAB + FLD_C_USED] += sum;
  QXCHK(qx::upload(f->stream, f->d_acc, acc.data(), FLD_ACC_WORDS * sizeof(u64)));
  QXCHK(qx::sync(f->stream));
  memcpy(f->h, acc.data() + FLD_SLAB, sizeof(f->h));
  f->units += (int64_t)sum;
  return QM_OK;
}

static int fld_stat(const qm_fld* f, int which, int64_t* value) {
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

#ifndef QM_EMU
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
  f->maxLen = max_len; f->maxBlocks = (int)(flags & 0xffffu);
  int rc = f->open("qm_fld_create", c->device, c->numCU);
  if (!rc && f->d_acc.ensure(FLD_ACC_WORDS) != QM_OK) rc = fail(QM_E_NOGPU, "qm_fld_create: stream / bins");
  if (!rc && fld_open(f) != QM_OK) rc = fail(QM_E_NOGPU, "qm_fld_create: memset");
  if (rc) { qm_fld_destroy(f); return rc; }
  *out = f;
  return QM_OK;
}

int qm_fld_destroy(qm_fld* f) {
  if (!f) return QM_OK;
  f->close();
  delete f;                    // (the buffers free themselves)
  return QM_OK;
}

int qm_fld_clear(qm_fld* f) {
  if (!f) return fail(QM_E_ARG, "null histogram");
  HIPCHK(hipSetDevice(f->device));
  return fld_clear(f);
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
  if (!f) return fail(QM_E_ARG, "qm_fld_add_hits: bad argument");
  HIPCHK(hipSetDevice(f->device));
  return fld_add_hits(f, n, offsets, hits, 1 << 22, 1 << 21);       // a part: what is uploaded and folded in one go
}

int qm_fld_fetch(qm_fld* f, uint64_t* counts) {
  if (!f || !counts) return fail(QM_E_ARG, "qm_fld_fetch: bad argument");
  HIPCHK(hipSetDevice(f->device));
  return fld_fetch(f, counts);
}

int qm_fld_add_counts(qm_fld* f, const uint64_t* counts) {
  if (!f || !counts) return fail(QM_E_ARG, "qm_fld_add_counts: bad argument");
  HIPCHK(hipSetDevice(f->device));
  return fld_add_counts(f, counts);
}

int qm_fld_stat(const qm_fld* f, int which, int64_t* value) {
  if (!f || !value) return fail(QM_E_ARG, "qm_fld_stat: bad argument");
  return fld_stat(f, which, value);
}

int qm_fld_eff_lens(qm_fld* f, int64_t n_txps, const uint32_t* lens, double* eff) {
  if (!f) return fail(QM_E_ARG, "qm_fld_eff_lens: null histogram");
  std::vector<uint64_t> counts((size_t)f->maxLen + 1);
  const int rc = qm_fld_fetch(f, counts.data());
  return rc ? rc : qm_fld_eff_lens_from_counts(f->maxLen, counts.data(), n_txps, lens, eff);
}

}  // extern "C"
#endif
