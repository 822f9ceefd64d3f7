// tests/emu/qm_emu_quant.cpp -- TEST-ONLY lane emulation of the abundance estimation: the driver of rapmap_amd/csrc/qm_quant_host.inl
// and the device code of qm_quant.inl, both compiled with -DQM_EMU (an LV<T> is a 64-entry array, QM_LANES a loop, a launch a loop
// over the wavefronts, a scan and a stable sort on the host: qm_exec.h).  What is here is the test's input -- its canonical arrays
// laid out as a table -- and a C face over the driver's object.  One wavefront after the other, one lane after the other: this
// checks the driver, the logic of the structure build and of the two iteration bodies (and the order of their sums), not the atomics.
#define QM_EMU
#include "../../rapmap_amd/csrc/qm_wave.h"
using namespace qm;
#include "../../rapmap_amd/csrc/qm_eqc_host.inl"
#include "../../rapmap_amd/csrc/qm_quant_host.inl"

namespace {
// nc classes in canonical arrays (off, tids, cnt) as a table at rest, with unpublished slots between the published ones
int table_of(qm_eqc& t, long long nc, const long long* off, const u32* tids, const u64* cnt) {
  const long long ne = off[nc];
  if (int rc = eqc_open(&t, (u64)(2 * nc + 5), (u64)std::max<long long>(ne, 1))) return rc;
  if (ne) memcpy(t.store.pool.p, tids, (size_t)ne * 4);
  for (long long c = 0; c < nc; ++c) { const size_t s = (size_t)(2 * c + 1); t.T.key[s] = 1ULL << 63; t.T.count[s] = cnt[c]; t.T.loff[s] = off[c]; t.T.llen[s] = (u32)(off[c + 1] - off[c]); }
  t.d_scal[EQC_SC_CLASSES] = (u64)nc; t.d_scal[EQC_SC_POOL] = (u64)ne;
  return QM_OK;
}
}  // namespace

extern "C" {

// eff: nTxps numbers or NULL (1.0 each).  *err: a QM_* code (QM_E_ARG when a label names a transcript >= nTxps, as on the device).
void* qe_quant_create(long long nc, const long long* off, const u32* tids, const u64* cnt, long long nTxps, const double* eff, int* err) {
  qm_eqc t;
  qm_quant* q = new qm_quant();
  if ((*err = quant_check(nTxps, eff)) || (*err = table_of(t, nc, off, tids, cnt)) || (*err = quant_open(q, &t, nTxps, eff))) { delete q; return nullptr; }
  return q;                                                           // (the object outlives its table)
}
int qe_quant_destroy(void* h) {
  qm_quant* q = (qm_quant*)h;
  if (int rc = quant_may_close(q)) return rc;
  delete q;
  return QM_OK;
}
int qe_quant_set_start(void* h, const double* alpha0) { return quant_set_start((qm_quant*)h, alpha0); }
int qe_quant_run(void* h, int max_iter, int check_every, double rel_tol, double min_alpha, int* iterations, double* rel) {
  return quant_run((qm_quant*)h, max_iter, check_every, rel_tol, min_alpha, iterations, rel);
}
int qe_quant_fetch(void* h, double* alpha) { return quant_fetch((qm_quant*)h, alpha); }
// stats: [0] classes [1] entries [2] present [3] longest label [4] longest list [5] queued labels [6] queued transcripts
void qe_quant_stats(void* h, long long* stats) {
  const qm_quant& q = *(qm_quant*)h;
  stats[0] = q.nClasses; stats[1] = q.nEntries; stats[2] = q.present; stats[3] = q.maxLabel; stats[4] = q.maxList; stats[5] = q.nqCls; stats[6] = q.nqTxp;
}

}  // extern "C"
