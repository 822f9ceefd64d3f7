// qm_fld_host.inl -- host driver of the fragment-length histogram (device code: qm_fld.inl; the tally half: qm_tally_host.inl) and
// the arithmetic from histogram to effective lengths.  Included at the end of qm_host.hip: qm_fld_add reads the context's last result
// where it lies in device memory.  Everything above the extern "C" block is written against qm_exec.h and compiled twice: here, and
// with -DQM_EMU by tests/emu.
//
// A fold = one launch of a persistent grid, then the six counters (and nothing else) read back: one host wait.  The effective
// lengths are host arithmetic over the fetched bins: once per run over 8 KB, off the per-batch path.
#include <algorithm>
#include "qm_fld.inl"
#include "qm_tally_host.inl"

struct qm_fld : qx::Tally<FLD_SLAB> {};

// (the driver's functions are what the extern "C" shells below and the emulation's face call)
static int fld_open(qm_fld* f) { return f->open_bins(); }
static int fld_clear(qm_fld* f) { return f->clear(); }

static int fld_fold(qm_fld* f, const UnitSrc& S, qx::Stream st) {
  return f->fold(S, st, FLD_BLOCKS_PER_CU, [&](const SweepAcc& A, int blocks) { return qx::sweep<fld_wave, FLD_SLAB>(st, blocks, S, A); });
}
// qm_fld_add_hits: the host arrays in parts (at most maxUnits units and maxHits hits each) through the fold
static int fld_add_hits(qm_fld* f, int64_t n, const int64_t* offsets, const qm_hit* hits, int64_t maxUnits, int64_t maxHits) {
  return f->add_hits("qm_fld_add_hits", n, offsets, hits, maxUnits, maxHits, [&](const UnitSrc& S) { return fld_fold(f, S, f->stream); });
}
static int fld_add_counts(qm_fld* f, const uint64_t* counts) {
  if (counts[0]) return fail(QM_E_ARG, "qm_fld_add_counts: bin 0 holds %llu", (unsigned long long)counts[0]);
  return f->add_counts(counts, f->maxLen + 1);
}

static int fld_stat(const qm_fld* f, int which, int64_t* value) {
  switch (which) {
    case QM_FLD_STAT_UNITS: *value = f->units; break;
    case QM_FLD_STAT_USED: *value = (int64_t)f->h[SW_C_USED]; break;
    case QM_FLD_STAT_UNMAPPED: *value = (int64_t)f->h[SW_C_UNMAPPED]; break;
    case QM_FLD_STAT_MULTI: *value = (int64_t)f->h[SW_C_MULTI]; break;
    case QM_FLD_STAT_NOT_PAIRED: *value = (int64_t)f->h[SW_C_NOT_PAIRED]; break;
    case QM_FLD_STAT_SAME_STRAND: *value = (int64_t)f->h[SW_C_SAME_STRAND]; break;
    case QM_FLD_STAT_OUT_OF_RANGE: *value = (int64_t)f->h[SW_C_OUT_OF_RANGE]; break;
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
  if (!rc && f->d_acc.ensure(FLD_SLAB + FLD_C_WORDS) != QM_OK) rc = fail(QM_E_NOGPU, "qm_fld_create: stream / bins");
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
  QXCHK(qx::enter(f, true, "null histogram"));
  return fld_clear(f);
}

int qm_fld_add(qm_fld* f, qm_ctx* c) {
  QXCHK(qx::enter_add(f, c, "qm_fld_add", "histogram", "fold"));
  return fld_fold(f, qx::last_units(c), c->stream);
}

int qm_fld_add_hits(qm_fld* f, int64_t n, const int64_t* offsets, const qm_hit* hits) {
  QXCHK(qx::enter(f, true, "qm_fld_add_hits: bad argument"));
  return fld_add_hits(f, n, offsets, hits, 1 << 22, 1 << 21);       // a part: what is uploaded and folded in one go
}

int qm_fld_fetch(qm_fld* f, uint64_t* counts) {
  QXCHK(qx::enter(f, counts != nullptr, "qm_fld_fetch: bad argument"));
  return f->fetch(counts, f->maxLen + 1);
}

int qm_fld_add_counts(qm_fld* f, const uint64_t* counts) {
  QXCHK(qx::enter(f, counts != nullptr, "qm_fld_add_counts: bad argument"));
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
