// tests/emu/qm_emu_eqc.cpp -- TEST-ONLY lane emulation of the equivalence-class table: the driver of rapmap_amd/csrc/qm_eqc_host.inl
// and the device code of qm_eqc.inl, both compiled with -DQM_EMU (an LV<T> is a 64-entry array, QM_LANES a loop, a launch a loop
// over the wavefronts: qm_exec.h).  What is here is a C face over the driver's object.  One wavefront after the other, one lane
// after the other: this checks the driver and the logic of the label and insert stages, not the atomics.
#define QM_EMU
#include "../../rapmap_amd/csrc/qm_wave.h"
using namespace qm;
#include "../../rapmap_amd/csrc/qm_eqc_host.inl"

extern "C" {

// Folds `folds` times the n lists (tids at `stride` bytes) into a fresh table of `cap` slots (a power of two) and `pool_cap` pool
// words; out_off needs room for as many classes as there are lists (+ 1), out_tids for off[n] words.  long_cap: capacity of the
// long-unit queue (a smaller one than the units need is grown after the count, as on the device).
// stats: [0] growths [1] collision probes [2] long units [3] rounds.  Returns the number of classes, or a QM_* code (negative).
long long qe_eqc_run(long long n, const long long* off, const unsigned char* tids, int stride, const u64* weights, int hash_bits, u64 cap, u64 pool_cap,
                     long long long_cap, int aggregate, int folds, long long* out_off, u32* out_tids, u64* out_counts, long long* stats) {
  qm_eqc t;
  t.aggregate = aggregate; t.keyMask = hash_bits ? ((1ULL << hash_bits) - 1) : ~0ULL; t.longMin = long_cap > 0 ? long_cap : 1;
  int rc = eqc_open(&t, cap, pool_cap);
  for (int f = 0; f < folds && !rc; ++f) {
    EqcSrc S{};
    S.tids = tids; S.stride = stride; S.off = off; S.n = n;
    rc = eqc_fold(&t, S, off[n], weights, t.stream);
  }
  long long nc = rc;
  if (!rc) {
    const EqcTable& T = t.T;
    std::vector<size_t> order;
    for (size_t s = 0; s <= T.mask; ++s) if (T.key[s]) order.push_back(s);
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
      return std::lexicographical_compare(T.pool + T.loff[a], T.pool + T.loff[a] + T.llen[a], T.pool + T.loff[b], T.pool + T.loff[b] + T.llen[b]);
    });
    long long o = 0;
    for (size_t i = 0; i < order.size(); ++i) {
      const size_t s = order[i];
      out_off[i] = o; memcpy(out_tids + o, T.pool + T.loff[s], (size_t)T.llen[s] * 4); out_counts[i] = T.count[s]; o += T.llen[s];
    }
    out_off[order.size()] = o;
    nc = (long long)order.size();
    if ((u64)nc != t.d_scal[EQC_SC_CLASSES] || (u64)o != t.d_scal[EQC_SC_POOL]) nc = QM_E_STATE;
  }
  stats[0] = t.growths; stats[1] = (long long)t.d_scal[EQC_SC_PROBES]; stats[2] = t.longUnits; stats[3] = t.rounds;
  return nc;
}

}  // extern "C"
