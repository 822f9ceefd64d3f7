// qm_eqc_host.inl -- host driver of the equivalence-class table (device code: qm_eqc.inl; the kernels that are no plain wave body:
// qm_kernels_eqc.hip).  Included at the end of qm_host.hip: qm_eqc_add reads the context's last result where it lies in device memory.
// Everything above the extern "C" block is written against qm_exec.h and compiled twice: here, and with -DQM_EMU by tests/emu.
//
// A fold = label launch (+ queue launch for the units of more than EQC_GROUP hits), then rounds of probe / publish until the
// pending queue is empty; the host reads the scalar block once per round.  When slots or pool run out (counted by the kernels,
// nothing written) the table is rebuilt four times as large -- the old table's slots go through the same probe / publish
// launches as units whose weights are their counts -- and the pending units start over.
#include <algorithm>
#include "qm_eqc.inl"
#include "qm_exec.h"

struct EqcStore {              // the six arrays of a table; EqcTable is a view of them
  DevBuf<u64> key, claim, count; DevBuf<long long> loff; DevBuf<u32> llen, pool;
  void swap(EqcStore& o) { key.swap(o.key); claim.swap(o.claim); count.swap(o.count); loff.swap(o.loff); llen.swap(o.llen); pool.swap(o.pool); }
};
struct qm_eqc : qx::Base {
  u64 keyMask = ~0ULL; int aggregate = 1;
  EqcStore store; EqcTable T{}; DevBuf<u64> d_scal; u64 h[EQC_SC_WORDS] = {0};
  // a fold's scratch
  DevBuf<u32> d_lab, d_len; DevBuf<u64> d_key, d_q[2]; DevBuf<long long> d_longq;
  int64_t longMin = 1024;                                             // the long-unit queue's least capacity (the emulation starts smaller: the regrow is tested)
  DevBuf<u64> d_gq[2];                                                // the queues of a rebuild
  qx::FeedBuf in;                                                     // qm_eqc_add_labels
  int64_t growths = 0, longUnits = 0, rounds = 0;
  int64_t lastFoldUs = 0;                                             // the events: around the last fold on its stream (QM_EQC_STAT_LAST_FOLD_US)
};

// the kernels that are no plain wave body (qm_kernels_eqc.hip, declared in qm_device.h), as the emulation runs them
#ifdef QM_EMU
static int qmk_eqc_label_queued(const EqcSrc& S, long long nq, qx::Stream) {
  std::vector<u32> slab(EQC_SLAB);
  for (long long w = 0; w < nq; ++w) eqc_label_queued(S, w, slab.data());
  return 0;
}
static int qmk_eqc_reset_probes(u64* q, long long n, qx::Stream) {
  for (long long i = 0; i < n; ++i) q[i] &= 0xffffffffULL;
  return 0;
}
static int qmk_eqc_sum(const u64* count, const u64* key, long long cap, u64* out, qx::Stream) {
  for (long long i = 0; i < cap; ++i) if (key[i]) *out += count[i];
  return 0;
}
#endif
// (the probe body takes the wavefront's index before its last argument)
QM_DEV void eqc_probe_body(const EqcTable& T, const EqcSet& S, const u64* qin, long long nin, u64* qout, int aggregate, long long wave) {
  eqc_probe_wave(T, S, qin, nin, qout, wave, aggregate);
}

static int eqc_clear_table(const EqcTable& T, qx::Stream st) {
  const u64 cap = T.mask + 1;
  QXCHK(qx::fill(st, T.key, 0, cap * 8)); QXCHK(qx::fill(st, T.llen, 0, cap * 4)); QXCHK(qx::fill(st, T.count, 0, cap * 8));
  return qx::fill(st, T.claim, 0xff, cap * 8);
}
// a cleared table of cap slots in `s`, and its view
static int eqc_alloc_table(qm_eqc* t, u64 cap, u64 poolCap, qx::Stream st, EqcStore& s, EqcTable& T) {
  if (s.key.ensure((int64_t)cap) || s.claim.ensure((int64_t)cap) || s.loff.ensure((int64_t)cap) || s.llen.ensure((int64_t)cap) || s.count.ensure((int64_t)cap) || s.pool.ensure((int64_t)poolCap))
    return fail(QM_E_NOMEM, "no device memory for an equivalence-class table of %llu slots", (unsigned long long)cap);
  T = EqcTable{s.key, s.claim, s.loff, s.llen, s.count, s.pool, cap - 1, cap / 2, poolCap, t->d_scal};
  return eqc_clear_table(T, st);
}
// the scalars and the first table of a new object
static int eqc_open(qm_eqc* t, u64 cap, u64 poolCap) {
  int rc;
  if ((rc = t->d_scal.ensure(EQC_SC_WORDS)) || (rc = qx::fill(t->stream, t->d_scal, 0, sizeof(t->h))) || (rc = eqc_alloc_table(t, cap, poolCap, t->stream, t->store, t->T))) return rc;
  return qx::sync(t->stream);
}
static int eqc_clear(qm_eqc* t) {
  int rc;
  if ((rc = eqc_clear_table(t->T, t->stream)) || (rc = qx::fill(t->stream, t->d_scal, 0, sizeof(t->h))) || (rc = qx::sync(t->stream))) return rc;
  memset(t->h, 0, sizeof(t->h));
  t->growths = t->longUnits = t->rounds = 0;
  return QM_OK;
}
static int eqc_read_scalars(qm_eqc* t, qx::Stream st) { return qx::read(st, t->h, t->d_scal, sizeof(t->h)); }

static int eqc_insert(qm_eqc* t, const EqcSet& S, qx::Stream st, u64** q, bool mayGrow);
static int eqc_grow(qm_eqc* t, qx::Stream st) {
  const EqcTable old = t->T;
  const u64 oldCap = old.mask + 1;
  const bool slots = t->h[EQC_SC_SLOT_OVF] || t->h[EQC_SC_FULL];
  // unit and slot indices travel as 32-bit numbers (queue entries, claim words)
  if (slots && oldCap >= (1ULL << 31)) return fail(QM_E_UNSUPPORTED, "equivalence-class table: more than 2^30 classes (a table cannot grow beyond 2^31 slots)");
  const u64 cap = slots ? (oldCap * 4 > (1ULL << 31) ? (1ULL << 31) : oldCap * 4) : oldCap, poolCap = t->h[EQC_SC_POOL_OVF] ? old.poolCap * 4 : old.poolCap;
  int rc;
  EqcStore s; EqcTable T;                                             // the new arrays; after the swap the old ones, freed on the way out
  if ((rc = eqc_alloc_table(t, cap, poolCap, st, s, T))) return rc;
  QXCHK(qx::fill(st, t->d_scal + EQC_SC_FULL, 0, 6 * sizeof(u64)));  // FULL, TICKETS, POOL, CLASSES and the two overflow counts
  t->store.swap(s); t->T = T;
  if ((rc = t->d_gq[0].ensure((int64_t)oldCap)) || (rc = t->d_gq[1].ensure((int64_t)oldCap))) return rc;
  const EqcSet R{old.pool, old.loff, old.llen, old.key, old.count, (long long)oldCap};     // empty slots have length 0: skipped like units without hits
  u64* gq[2] = {t->d_gq[0], t->d_gq[1]};
  rc = eqc_insert(t, R, st, gq, false);
  t->growths++;
  return rc;
}

// every unit of S into the table; q: two queues of S.n entries each
static int eqc_insert(qm_eqc* t, const EqcSet& S, qx::Stream st, u64** q, bool mayGrow) {
  const u64* qin = nullptr; long long nin = S.n; int cur = 0, rc;
  for (long long guard = 0;; ++guard) {
    if (guard > (1LL << 40)) return fail(QM_E_STATE, "equivalence-class insert does not end");
    QXCHK(qx::fill(st, t->d_scal + EQC_SC_PEND, 0, 2 * sizeof(u64)));   // PEND, FULL
    HIPCHK(qx::launch<eqc_probe_body>(st, qx::waves_of(nin), t->T, S, qin, nin, q[cur], t->aggregate));
    t->rounds++;
    if ((rc = eqc_read_scalars(t, st))) return rc;
    const long long pend = (long long)t->h[EQC_SC_PEND];
    if (!pend) return QM_OK;
    if (t->h[EQC_SC_SLOT_OVF] || t->h[EQC_SC_POOL_OVF] || t->h[EQC_SC_FULL]) {
      if (!mayGrow) return fail(QM_E_STATE, "equivalence-class table overflowed while it was rebuilt");
      if ((rc = eqc_grow(t, st))) return rc;
      HIPCHK(qmk_eqc_reset_probes(q[cur], pend, st));
    }
    else HIPCHK(qx::launch<eqc_publish_wave>(st, qx::waves_of(pend), t->T, S, (const u64*)q[cur], pend));
    qin = q[cur]; nin = pend; cur ^= 1;
  }
}

// S: tids, stride, off, n filled in; nTids = off[n] (off[0] = 0)
static int eqc_fold(qm_eqc* t, EqcSrc S, int64_t nTids, const u64* d_w, qx::Stream st) {
  if (S.n <= 0 || nTids <= 0) return QM_OK;
  if (S.n >= (1LL << 32)) return fail(QM_E_ARG, "more than 2^32 - 1 units in one fold");
  int rc;
  if ((rc = t->d_lab.ensure(nTids)) || (rc = t->d_len.ensure(S.n)) || (rc = t->d_key.ensure(S.n)) ||
      (rc = t->d_q[0].ensure(S.n)) || (rc = t->d_q[1].ensure(S.n)) || (rc = t->d_longq.ensure(std::max<int64_t>(t->longMin, S.n / 16)))) return rc;
  S.lab = t->d_lab; S.len = t->d_len; S.key = t->d_key; S.scal = t->d_scal; S.keyMask = t->keyMask;
  if ((rc = qx::tick(t->ev0, st))) return rc;
  int64_t nl = 0;
  for (int pass = 0;; ++pass) {
    S.longq = t->d_longq; S.longCap = (u64)t->d_longq.cap;
    QXCHK(qx::fill(st, t->d_scal + EQC_SC_LONGQ, 0, sizeof(u64)));
    HIPCHK(qx::launch<eqc_label_wave>(st, (S.n + 64 / EQC_GROUP - 1) / (64 / EQC_GROUP), S));
    if ((rc = eqc_read_scalars(t, st))) return rc;
    nl = (int64_t)t->h[EQC_SC_LONGQ];
    if (nl <= t->d_longq.cap) break;
    if (pass) return fail(QM_E_STATE, "long-unit queue overflowed twice");
    if ((rc = t->d_longq.ensure(nl))) return rc;       // counted, not written: a larger queue and the launch again
  }
  HIPCHK(qmk_eqc_label_queued(S, nl, st));
  t->longUnits += nl;
  const EqcSet set{S.lab, S.off, S.len, S.key, d_w, S.n};
  u64* q[2] = {t->d_q[0], t->d_q[1]};
  if ((rc = eqc_insert(t, set, st, q, true))) return rc;
  return qx::tock(t->ev0, t->ev1, st, &t->lastFoldUs);              // (the stream is idle: the insert ended with a read-back)
}

// the counters of the table; with total_count the sum of the published slots' counts (one launch more)
static int eqc_size(qm_eqc* t, int64_t* n_classes, int64_t* n_tids, uint64_t* total_count) {
  if (total_count) {
    QXCHK(qx::fill(t->stream, t->d_scal + EQC_SC_SUM, 0, sizeof(u64)));
    HIPCHK(qmk_eqc_sum(t->T.count, t->T.key, (long long)(t->T.mask + 1), t->d_scal + EQC_SC_SUM, t->stream));
  }
  int rc;
  if ((rc = eqc_read_scalars(t, t->stream))) return rc;
  if (n_classes) *n_classes = (int64_t)t->h[EQC_SC_CLASSES];
  if (n_tids) *n_tids = (int64_t)t->h[EQC_SC_POOL];             // (exact: a fold that ran out of pool rebuilt the table)
  if (total_count) *total_count = t->h[EQC_SC_SUM];
  return QM_OK;
}

// qm_eqc_add_labels: the host lists in parts (at most maxUnits lists and maxTids tids each) through the fold
static int eqc_add_labels(qm_eqc* t, int64_t n, const int64_t* offsets, const uint32_t* tids, const uint64_t* weights, int64_t maxUnits, int64_t maxTids) {
  return qx::feed(t->stream, t->in, "qm_eqc_add_labels", "list", "tids", n, offsets, tids, 4, weights, maxUnits, maxTids,
                  [&](const long long* off, const unsigned char* d_tids, const u64* d_w, int64_t, int64_t nu, int64_t nt) {
                    EqcSrc S{};
                    S.tids = d_tids; S.stride = 4; S.off = off; S.n = nu;
                    return eqc_fold(t, S, nt, d_w, t->stream);
                  });
}

// The table in canonical order as CSR arrays (label_offsets: classes + 1 entries; tids, counts: may be null): the published slots,
// labels ascending, compared as sequences of unsigned 32-bit numbers (a proper prefix comes first).  t->h holds the scalars afterwards.
static int eqc_fetch(qm_eqc* t, int64_t* label_offsets, uint32_t* tids, uint64_t* counts) {
  int rc;
  if ((rc = eqc_read_scalars(t, t->stream))) return rc;
  const size_t cap = (size_t)(t->T.mask + 1), used = (size_t)t->h[EQC_SC_POOL];
  std::vector<u64> key(cap), cnt(cap); std::vector<long long> loff(cap); std::vector<u32> llen(cap), pool(used + 1);
  if ((rc = qx::read(t->stream, key.data(), t->T.key, cap * 8)) || (rc = qx::read(t->stream, cnt.data(), t->T.count, cap * 8)) ||
      (rc = qx::read(t->stream, loff.data(), t->T.loff, cap * 8)) || (rc = qx::read(t->stream, llen.data(), t->T.llen, cap * 4)) ||
      (used && (rc = qx::read(t->stream, pool.data(), t->T.pool, used * 4)))) return rc;
  std::vector<size_t> order;
  for (size_t s = 0; s < cap; ++s) if (key[s]) order.push_back(s);
  if (order.size() != (size_t)t->h[EQC_SC_CLASSES]) return fail(QM_E_STATE, "equivalence-class table: %zu published slots, %llu counted", order.size(), (unsigned long long)t->h[EQC_SC_CLASSES]);
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    return std::lexicographical_compare(pool.begin() + loff[a], pool.begin() + loff[a] + llen[a], pool.begin() + loff[b], pool.begin() + loff[b] + llen[b]);
  });
  int64_t o = 0;
  for (size_t i = 0; i < order.size(); ++i) {
    const size_t s = order[i];
    label_offsets[i] = o;
    if (tids) memcpy(tids + o, pool.data() + loff[s], (size_t)llen[s] * 4);
    if (counts) counts[i] = cnt[s];
    o += llen[s];
  }
  label_offsets[order.size()] = o;
  return QM_OK;
}

#ifndef QM_EMU
extern "C" {

int qm_eqc_create(qm_ctx* c, int64_t expected_classes, uint32_t flags, qm_eqc** out) {
  if (!c || !out || expected_classes < 0 || (flags & ~0xff00u)) return fail(QM_E_ARG, "qm_eqc_create: bad argument");
  const int bits = (int)((flags >> 8) & 0xff);
  if (bits > 63) return fail(QM_E_ARG, "qm_eqc_create: at most 63 key bits");
  HIPCHK(hipSetDevice(c->device));
  qm_eqc* t = new qm_eqc();
  t->keyMask = bits ? ((1ULL << bits) - 1) : ~0ULL;
  { const char* e = getenv("QM_EQC_NO_AGGREGATE"); t->aggregate = !(e && atoi(e) != 0); }   // (A/B timing of the per-wavefront aggregation: INTEGRATION.md, environment)
  u64 cap = 16; while (cap < 2 * (u64)expected_classes && cap < (1ULL << 31)) cap <<= 1;
  int rc = t->open("qm_eqc_create", c->device, c->numCU);
  if (!rc) rc = eqc_open(t, cap, std::max<u64>(64, 8 * (u64)expected_classes));
  if (rc) { qm_eqc_destroy(t); return rc; }
  *out = t;
  return QM_OK;
}

int qm_eqc_destroy(qm_eqc* t) {
  if (!t) return QM_OK;
  t->close();
  delete t;                    // (the table and the scratch buffers free themselves)
  return QM_OK;
}

int qm_eqc_clear(qm_eqc* t) {
  if (!t) return fail(QM_E_ARG, "null table");
  HIPCHK(hipSetDevice(t->device));
  return eqc_clear(t);
}

int qm_eqc_add(qm_eqc* t, qm_ctx* c) {
  if (!t || !c) return fail(QM_E_ARG, "qm_eqc_add: null argument");
  if (c->last.units < 0) return fail(QM_E_STATE, "no mapping result to fold");
  if (c->device != t->device) return fail(QM_E_ARG, "table on device %d, context on device %d", t->device, c->device);
  HIPCHK(hipSetDevice(t->device));
  EqcSrc S{};
  S.tids = (const unsigned char*)c->d_hits.p; S.stride = (int)sizeof(qm_hit); S.off = c->d_offs; S.n = c->last.units;
  return eqc_fold(t, S, c->last.hits, nullptr, c->stream);
}

int qm_eqc_add_labels(qm_eqc* t, int64_t n, const int64_t* offsets, const uint32_t* tids, const uint64_t* weights) {
  if (!t) return fail(QM_E_ARG, "qm_eqc_add_labels: bad argument");
  HIPCHK(hipSetDevice(t->device));
  return eqc_add_labels(t, n, offsets, tids, weights, 1 << 22, 1 << 25);   // a part: what is uploaded and folded in one go
}

int qm_eqc_size(qm_eqc* t, int64_t* n_classes, int64_t* n_tids, uint64_t* total_count) {
  if (!t) return fail(QM_E_ARG, "null table");
  HIPCHK(hipSetDevice(t->device));
  return eqc_size(t, n_classes, n_tids, total_count);
}

int qm_eqc_fetch(qm_eqc* t, int64_t* label_offsets, uint32_t* tids, uint64_t* counts) {
  if (!t || !label_offsets) return fail(QM_E_ARG, "qm_eqc_fetch: bad argument");
  HIPCHK(hipSetDevice(t->device));
  return eqc_fetch(t, label_offsets, tids, counts);
}

int qm_eqc_stat(const qm_eqc* t, int which, int64_t* value) {
  if (!t || !value) return fail(QM_E_ARG, "qm_eqc_stat: bad argument");
  switch (which) {
    case QM_EQC_STAT_GROWTHS: *value = t->growths; break;
    case QM_EQC_STAT_COLLISION_PROBES: *value = (int64_t)t->h[EQC_SC_PROBES]; break;
    case QM_EQC_STAT_LONG_UNITS: *value = t->longUnits; break;
    case QM_EQC_STAT_ROUNDS: *value = t->rounds; break;
    case QM_EQC_STAT_LAST_FOLD_US: *value = t->lastFoldUs; break;
    default: return fail(QM_E_ARG, "qm_eqc_stat: unknown statistic %d", which);
  }
  return QM_OK;
}

}  // extern "C"
#endif
