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
// long-unit queue (a smaller one than the units need is grown after the count, as on the device).  max_units > 0: the lists are host
// arrays (stride 4; off[0] need not be 0) and go through qm_eqc_add_labels' driver in parts of at most max_units lists and max_tids tids.
// stats: [0] growths [1] collision probes [2] long units [3] rounds.  Returns the number of classes, or a QM_* code (negative).
long long qe_eqc_run(long long n, const int64_t* off, const unsigned char* tids, int stride, const uint64_t* weights, int hash_bits, u64 cap, u64 pool_cap,
                     long long long_cap, int aggregate, int folds, long long max_units, long long max_tids, int64_t* out_off, u32* out_tids, uint64_t* out_counts,
                     long long* stats) {
  qm_eqc t;
  t.aggregate = aggregate; t.keyMask = hash_bits ? ((1ULL << hash_bits) - 1) : ~0ULL; t.longMin = long_cap > 0 ? long_cap : 1;
  int rc = eqc_open(&t, cap, pool_cap);
  for (int f = 0; f < folds && !rc; ++f) {
    if (max_units > 0) { rc = stride == 4 ? eqc_add_labels(&t, n, off, (const u32*)tids, weights, max_units, max_tids) : QM_E_ARG; continue; }
    EqcSrc S{};
    S.tids = tids; S.stride = stride; S.off = (const long long*)off; S.n = n;
    rc = eqc_fold(&t, S, off[n], (const u64*)weights, t.stream);
  }
  if (!rc) rc = eqc_fetch(&t, out_off, out_tids, out_counts);
  long long nc = rc;
  if (!rc) {
    nc = (long long)t.h[EQC_SC_CLASSES];
    if ((u64)out_off[nc] != t.d_scal[EQC_SC_POOL]) nc = QM_E_STATE;   // (eqc_fetch holds the published slots to the counted classes; here: the pool's total)
  }
  stats[0] = t.growths; stats[1] = (long long)t.d_scal[EQC_SC_PROBES]; stats[2] = t.longUnits; stats[3] = t.rounds;
  return nc;
}

}  // extern "C"
