// qm_tally_host.inl -- the tally half of a driver whose object is bins plus counters filled by a sweep of qm_sweep.h (qm_fld_host.inl,
// qm_gcb_host.inl), and the preambles of the extern "C" shells of every per-batch tally.  Written against qm_exec.h and compiled
// twice like the drivers: in qm_host.hip, and with -DQM_EMU by tests/emu.
#pragma once
#include "qm_sweep.h"
#include "qm_exec.h"
#include "qm_grid.h"

namespace qm {
namespace qx {

// BINS 64-bit bins, then the SW_C_WORDS counters, in one device buffer; the counters as last read; what qm_*_add_hits uploads into.
// A fold = tick, the sweep's launch, tick, the counters (and nothing else) read back -- the one host wait of a fold --, elapsed.
template <int BINS>
struct Tally : Base {
  int maxLen = QM_FLD_DEFAULT_MAX_LEN, maxBlocks = 0;
  DevBuf<u64> d_acc;
  u64 h[SW_C_WORDS] = {0};
  FeedBuf in;
  int64_t units = 0, folds = 0, lastFoldUs = 0;                       // (the events: around the last fold's kernel on its stream)

  int clear() {
    int rc;
    if ((rc = fill(stream, d_acc, 0, (BINS + SW_C_WORDS) * sizeof(u64))) || (rc = sync(stream))) return rc;
    memset(h, 0, sizeof(h));
    units = folds = lastFoldUs = 0;
    return QM_OK;
  }
  int open_bins() {
    const int rc = d_acc.ensure(BINS + SW_C_WORDS);
    return rc ? rc : clear();
  }
  // launch(acc, blocks) -> what HIPCHK takes; residentPerCU: the sweep's workgroups resident per compute unit
  template <class Launch>
  int fold(const UnitSrc& S, Stream st, int residentPerCU, Launch&& launch) {
    if (S.n <= 0) return QM_OK;
    if (S.n >= (1LL << 32)) return fail(QM_E_ARG, "more than 2^32 - 1 units in one fold");   // (a wavefront's 32-bit bins cannot overflow)
    QXCHK(tick(ev0, st));
    HIPCHK(launch(SweepAcc{d_acc, d_acc + BINS, maxLen}, sweep_grid(S.n, numCU, residentPerCU, maxBlocks)));
    QXCHK(tick(ev1, st));
    QXCHK(read(st, h, d_acc + BINS, sizeof(h)));                       // (the one wait of a fold: both events have passed)
    elapsed(ev0, ev1, &lastFoldUs);
    units += S.n; folds++;
    return QM_OK;
  }
  // the host arrays in parts (at most maxUnits units and maxHits hits each) through foldPart(src)
  template <class Fold>
  int add_hits(const char* who, int64_t n, const int64_t* offsets, const qm_hit* hits, int64_t maxUnits, int64_t maxHits, Fold&& foldPart) {
    return feed(stream, in, who, "unit", "hits", n, offsets, hits, sizeof(qm_hit), nullptr, maxUnits, maxHits,
                [&](const long long* off, const unsigned char* hp, const u64*, int64_t, int64_t nu, int64_t nh) {
                  return foldPart(UnitSrc{hp, (int)sizeof(qm_hit), off, nu, nh});
                });
  }
  int fetch(uint64_t* out, int nBins) { return read(stream, out, d_acc, (size_t)nBins * sizeof(u64)); }
  // off the per-batch path: the bins and the `used` counter come to the host, are added to and go back
  int add_counts(const uint64_t* counts, int nBins) {
    std::vector<u64> acc(BINS + SW_C_WORDS);
    QXCHK(read(stream, acc.data(), d_acc, acc.size() * sizeof(u64)));
    u64 sum = 0;
    for (int b = 0; b < nBins; ++b) { acc[(size_t)b] += counts[b]; sum += counts[b]; }
    acc[BINS + SW_C_USED] += sum;
    QXCHK(upload(stream, d_acc, acc.data(), acc.size() * sizeof(u64)));
    QXCHK(sync(stream));
    memcpy(h, acc.data() + BINS, sizeof(h));
    units += (int64_t)sum;
    return QM_OK;
  }
};

#ifndef QM_EMU
// the preamble of a shell that works on an object: `msg` when the object or another argument is missing, then its device
inline int enter(const Base* o, bool argsOk, const char* msg) {
  if (!o || !argsOk) return fail(QM_E_ARG, "%s", msg);
  HIPCHK(hipSetDevice(o->device));
  return QM_OK;
}
// ... of one that works on a context's last result where it lies: who: the function, what: the object in words, verb: what it does
inline int enter_add(const Base* o, const qm_ctx* c, const char* who, const char* what, const char* verb) {
  if (!o || !c) return fail(QM_E_ARG, "%s: null argument", who);
  if (c->last.units < 0) return fail(QM_E_STATE, "no mapping result to %s", verb);
  if (c->device != o->device) return fail(QM_E_ARG, "%s on device %d, context on device %d", what, o->device, c->device);
  HIPCHK(hipSetDevice(o->device));
  return QM_OK;
}
// the units of the context's last result
inline UnitSrc last_units(const qm_ctx* c) { return UnitSrc{(const unsigned char*)c->d_hits.p, (int)sizeof(qm_hit), c->d_offs, c->last.units, c->last.hits}; }
#endif

}  // namespace qx
}  // namespace qm
