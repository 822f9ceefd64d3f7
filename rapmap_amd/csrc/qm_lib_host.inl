// qm_lib_host.inl -- host driver of the library-type sweep (device code: qm_lib.inl; the shells' preambles: qm_tally_host.inl).
// Included at the end of qm_host.hip, after qm_eqc_host.inl: qm_lib_add reads the context's last result where it lies in device
// memory, qm_eqc_add_lib hands the compacted lists to eqc_fold.  Everything above the extern "C" block is written against
// qm_exec.h and compiled twice: here, and with -DQM_EMU by tests/emu.
//
// A sweep = classify launch (one lane per hit: tallies, keepMask, keepCnt), a scan of keepCnt into waveBase, the compaction launch
// when the caller wants the kept tids, and the unit launch (one lane per unit: new offsets, unit tallies).  12 bytes of scratch per
// 64 hits.  Nothing is read back but what the caller asks for.
#include <algorithm>
#include "qm_lib.inl"
#include "qm_tally_host.inl"

struct qm_lib : qx::Base {
  int maxBlocks = 0; u32 mask = LIB_ALL_CODES;
  DevBuf<u64> d_ctr;                                                  // LIB_WORDS
  DevBuf<u64> d_keepMask; DevBuf<u32> d_keepCnt; DevBuf<long long> d_waveBase; DevBuf<unsigned char> d_tmp;   // a sweep's scratch
  DevBuf<u32> d_outTids; DevBuf<long long> d_newOff;                  // the filtered lists of the last compacting sweep
  qx::FeedBuf in;                                                     // qm_lib_add_hits, qm_lib_compact_hits
  int64_t sweeps = 0, lastSweepUs = 0;                                // (the events: around the last sweep on its stream)
};

// the grid of the two persistent kernels over `lanes` hits or units (sweep_grid of qm_grid.h at this sweep's resident blocks)
static int qmk_lib_grid(long long lanes, int num_cu, int max_blocks) { return sweep_grid(lanes, num_cu, LIB_BLOCKS_PER_CU, max_blocks); }
static int lib_open(qm_lib* L) {
  int rc;
  if ((rc = L->d_ctr.ensure(LIB_WORDS)) || (rc = qx::fill(L->stream, L->d_ctr, 0, LIB_WORDS * sizeof(u64)))) return rc;
  return qx::sync(L->stream);
}
static int lib_clear(qm_lib* L) {
  int rc;
  if ((rc = qx::fill(L->stream, L->d_ctr, 0, LIB_WORDS * sizeof(u64))) || (rc = qx::sync(L->stream))) return rc;
  L->sweeps = L->lastSweepUs = 0;
  return QM_OK;
}

// S: hits, stride, off, n, nh filled in.  lists: the kept hits' tids go to d_outTids and the units' offsets to d_newOff.  The stream
// is idle when this returns.
static int lib_sweep(qm_lib* L, const UnitSrc& S, bool lists, qx::Stream st) {
  if (S.n <= 0) return QM_OK;
  if (S.n >= (1LL << 32)) return fail(QM_E_ARG, "more than 2^32 - 1 units in one sweep");
  const long long hw = qx::waves_of(S.nh);
  int rc;
  if ((rc = L->d_keepMask.ensure(hw + 1)) || (rc = L->d_keepCnt.ensure(hw + 1)) || (rc = L->d_waveBase.ensure(hw + 1))) return rc;
  if (lists && ((rc = L->d_outTids.ensure(std::max<int64_t>(S.nh, 1))) || (rc = L->d_newOff.ensure(S.n + 1)))) return rc;
  const LibAcc A{L->d_ctr, L->mask, L->d_keepMask, L->d_keepCnt, L->d_waveBase, lists ? L->d_outTids.p : nullptr, lists ? L->d_newOff.p : nullptr};
  if ((rc = qx::tick(L->ev0, st))) return rc;
  QXCHK(qx::fill(st, L->d_keepCnt + hw, 0, sizeof(u32)));            // (the scan's last input: read, never used)
  if (S.nh > 0) HIPCHK((qx::sweep<lib_classify_wave>(st, qmk_lib_grid(S.nh, L->numCU, L->maxBlocks), S, A)));
  QXCHK(qx::scan_u32(st, L->d_tmp, L->d_keepCnt, L->d_waveBase, hw + 1));
  if (lists) HIPCHK(qx::launch<lib_compact_wave>(st, hw, S, A));
  HIPCHK((qx::sweep<lib_units_wave>(st, qmk_lib_grid(S.n, L->numCU, L->maxBlocks), S, A)));
  if ((rc = qx::tock(L->ev0, L->ev1, st, &L->lastSweepUs))) return rc;
  L->sweeps++;
  return QM_OK;
}

// the fold of qm_eqc_add_lib: sweep, then eqc_fold over the filtered lists (the all-codes mask: nothing is compacted, the fold is
// qm_eqc_add's over the hits as they are)
static int lib_eqc_fold(qm_lib* L, qm_eqc* t, const UnitSrc& S, qx::Stream st) {
  int rc;
  if ((rc = lib_sweep(L, S, L->mask != LIB_ALL_CODES, st))) return rc;
  EqcSrc E{};
  E.n = S.n;
  if (L->mask == LIB_ALL_CODES) {
    E.tids = S.hits; E.stride = S.stride; E.off = S.off;
    return eqc_fold(t, E, S.nh, nullptr, st);
  }
  if (S.n <= 0) return QM_OK;
  long long kept = 0;
  if ((rc = qx::read(st, &kept, L->d_newOff + S.n, sizeof(kept)))) return rc;
  E.tids = (const unsigned char*)L->d_outTids.p; E.stride = 4; E.off = L->d_newOff;
  return eqc_fold(t, E, kept, nullptr, st);
}

// qm_lib_add_hits / qm_lib_compact_hits: the host arrays in parts (at most maxUnits units and maxHits hits each) through the sweep;
// with new_offsets every part's filtered lists are appended to new_offsets / tids
static int lib_add_host(qm_lib* L, const char* who, int64_t n, const int64_t* offsets, const qm_hit* hits, int64_t* new_offsets, uint32_t* tids,
                        int64_t maxUnits, int64_t maxHits) {
  int64_t outBase = 0;
  std::vector<long long> off;
  const int rc = qx::feed(L->stream, L->in, who, "unit", "hits", n, offsets, hits, sizeof(qm_hit), nullptr, maxUnits, maxHits,
                          [&](const long long* d_off, const unsigned char* d_hits, const u64*, int64_t u0, int64_t nu, int64_t nh) {
    QXCHK(lib_sweep(L, UnitSrc{d_hits, (int)sizeof(qm_hit), d_off, nu, nh}, new_offsets != nullptr, L->stream));
    if (!new_offsets) return (int)QM_OK;
    off.resize((size_t)nu + 1);
    QXCHK(qx::read(L->stream, off.data(), L->d_newOff, (size_t)(nu + 1) * 8));
    const long long kept = off[(size_t)nu];
    for (int64_t i = 1; i <= nu; ++i) new_offsets[u0 + i] = outBase + off[(size_t)i];
    if (kept > 0) {
      if (!tids) return fail(QM_E_ARG, "%s: null tids", who);
      QXCHK(qx::read(L->stream, tids + outBase, L->d_outTids, (size_t)kept * 4));
    }
    outBase += kept;
    return (int)QM_OK;
  });
  if (!rc && new_offsets) new_offsets[0] = 0;
  return rc;
}

#ifndef QM_EMU
#define LIB_PART_UNITS (1 << 22)   // a part of host arrays: what is uploaded and swept in one go
#define LIB_PART_HITS (1 << 21)

extern "C" {

int qm_lib_type_mask(const char* name, uint32_t* mask) {
  static const struct { const char* name; uint32_t mask; } types[] = {
    {"IU", 1u << LIB_ISF | 1u << LIB_ISR | 1u << LIB_LF | 1u << LIB_LR | 1u << LIB_RF | 1u << LIB_RR}, {"ISF", 1u << LIB_ISF | 1u << LIB_LF | 1u << LIB_RR},
    {"ISR", 1u << LIB_ISR | 1u << LIB_LR | 1u << LIB_RF},
    {"OU", 1u << LIB_OSF | 1u << LIB_OSR | 1u << LIB_LF | 1u << LIB_LR | 1u << LIB_RF | 1u << LIB_RR}, {"OSF", 1u << LIB_OSF | 1u << LIB_LF | 1u << LIB_RR},
    {"OSR", 1u << LIB_OSR | 1u << LIB_LR | 1u << LIB_RF},
    {"MU", 1u << LIB_MSF | 1u << LIB_MSR | 1u << LIB_LF | 1u << LIB_LR | 1u << LIB_RF | 1u << LIB_RR}, {"MSF", 1u << LIB_MSF | 1u << LIB_LF | 1u << LIB_RF},
    {"MSR", 1u << LIB_MSR | 1u << LIB_LR | 1u << LIB_RR},
    {"U", 1u << LIB_SF | 1u << LIB_SR}, {"SF", 1u << LIB_SF}, {"SR", 1u << LIB_SR}, {"A", LIB_ALL_CODES}};
  if (!name || !mask) return fail(QM_E_ARG, "qm_lib_type_mask: null argument");
  for (const auto& t : types) if (!strcmp(name, t.name)) { *mask = t.mask; return QM_OK; }
  return fail(QM_E_ARG, "qm_lib_type_mask: unknown library type '%s'", name);
}

int qm_lib_infer(const uint64_t counts[32], char out[4]) {
  if (!counts || !out) return fail(QM_E_ARG, "qm_lib_infer: null argument");
  const uint64_t* c = counts + LIB_W_SINGLE_BY_CODE;
  for (int i = 0; i < LIB_CODES; ++i) if (c[i] >= (1ULL << 59)) return fail(QM_E_UNSUPPORTED, "qm_lib_infer: a count of 2^59 or more");
  static const struct { int f, r; const char* name; } orient[4] = {{LIB_ISF, LIB_ISR, "I"}, {LIB_OSF, LIB_OSR, "O"}, {LIB_MSF, LIB_MSR, "M"}, {LIB_SF, LIB_SR, ""}};
  int best = 0;
  for (int i = 1; i < 4; ++i) if (c[orient[i].f] + c[orient[i].r] > c[orient[best].f] + c[orient[best].r]) best = i;   // (ties: the earlier one)
  const uint64_t a = c[orient[best].f], b = c[orient[best].r];
  memset(out, 0, 4);
  if (a + b == 0) return QM_OK;
  const char* sense = 10 * a > 7 * (a + b) ? "SF" : 10 * a < 3 * (a + b) ? "SR" : "U";
  snprintf(out, 4, "%s%s", orient[best].name, sense);
  return QM_OK;
}

int qm_lib_create(qm_ctx* c, uint32_t mask, uint32_t flags, qm_lib** out) {
  if (!c || !out || (flags & ~0xffffu)) return fail(QM_E_ARG, "qm_lib_create: bad argument");
  if (!mask || (mask & ~LIB_ALL_CODES)) return fail(QM_E_ARG, "qm_lib_create: mask 0x%x", (unsigned)mask);
  HIPCHK(hipSetDevice(c->device));
  qm_lib* L = new qm_lib();
  L->mask = mask; L->maxBlocks = (int)(flags & 0xffffu);
  int rc = L->open("qm_lib_create", c->device, c->numCU);
  if (!rc) rc = lib_open(L);
  if (rc) { qm_lib_destroy(L); return rc; }
  *out = L;
  return QM_OK;
}

int qm_lib_destroy(qm_lib* L) {
  if (!L) return QM_OK;
  L->close();
  delete L;                    // (the buffers free themselves)
  return QM_OK;
}

int qm_lib_clear(qm_lib* L) {
  QXCHK(qx::enter(L, true, "null library-type object"));
  return lib_clear(L);
}

int qm_lib_add(qm_lib* L, qm_ctx* c) {
  QXCHK(qx::enter_add(L, c, "qm_lib_add", "library-type object", "tally"));
  return lib_sweep(L, qx::last_units(c), false, c->stream);
}

int qm_lib_add_hits(qm_lib* L, int64_t n, const int64_t* offsets, const qm_hit* hits) {
  QXCHK(qx::enter(L, true, "qm_lib_add_hits: bad argument"));
  return lib_add_host(L, "qm_lib_add_hits", n, offsets, hits, nullptr, nullptr, LIB_PART_UNITS, LIB_PART_HITS);
}

int qm_lib_compact_hits(qm_lib* L, int64_t n, const int64_t* offsets, const qm_hit* hits, int64_t* new_offsets, uint32_t* tids) {
  if (!new_offsets) return fail(QM_E_ARG, "qm_lib_compact_hits: null new_offsets");
  QXCHK(qx::enter(L, true, "qm_lib_compact_hits: bad argument"));
  return lib_add_host(L, "qm_lib_compact_hits", n, offsets, hits, new_offsets, tids, LIB_PART_UNITS, LIB_PART_HITS);
}

int qm_lib_fetch(qm_lib* L, uint64_t counts[32]) {
  QXCHK(qx::enter(L, counts != nullptr, "qm_lib_fetch: bad argument"));
  return qx::read(L->stream, counts, L->d_ctr, LIB_WORDS * sizeof(u64));
}

int qm_lib_add_counts(qm_lib* L, const uint64_t counts[32]) {
  if (!L || !counts) return fail(QM_E_ARG, "qm_lib_add_counts: bad argument");
  if (counts[31]) return fail(QM_E_ARG, "qm_lib_add_counts: word 31 holds %llu", (unsigned long long)counts[31]);
  HIPCHK(hipSetDevice(L->device));
  // off the per-batch path: the tallies come to the host, are added to and go back
  u64 acc[LIB_WORDS];
  int rc;
  if ((rc = qx::read(L->stream, acc, L->d_ctr, sizeof(acc)))) return rc;
  for (int i = 0; i < LIB_WORDS; ++i) acc[i] += counts[i];
  if ((rc = qx::upload(L->stream, L->d_ctr, acc, sizeof(acc)))) return rc;
  return qx::sync(L->stream);
}

int qm_lib_stat(const qm_lib* L, int which, int64_t* value) {
  if (!L || !value) return fail(QM_E_ARG, "qm_lib_stat: bad argument");
  switch (which) {
    case QM_LIB_STAT_SWEEPS: *value = L->sweeps; break;
    case QM_LIB_STAT_LAST_SWEEP_US: *value = L->lastSweepUs; break;
    case QM_LIB_STAT_MASK: *value = (int64_t)L->mask; break;
    default: return fail(QM_E_ARG, "qm_lib_stat: unknown statistic %d", which);
  }
  return QM_OK;
}

int qm_eqc_add_lib(qm_eqc* t, qm_ctx* c, qm_lib* L) {
  if (!t || !c || !L) return fail(QM_E_ARG, "qm_eqc_add_lib: null argument");
  if (c->last.units < 0) return fail(QM_E_STATE, "no mapping result to fold");
  if (c->device != t->device || c->device != L->device) return fail(QM_E_ARG, "table on device %d, library-type object on device %d, context on device %d", t->device, L->device, c->device);
  HIPCHK(hipSetDevice(t->device));
  return lib_eqc_fold(L, t, qx::last_units(c), c->stream);
}

}  // extern "C"
#endif
