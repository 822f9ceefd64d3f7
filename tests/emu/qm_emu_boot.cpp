// tests/emu/qm_emu_boot.cpp -- TEST-ONLY lane emulation of the bootstrap replicates: the driver of rapmap_amd/csrc/qm_boot_host.inl
// and the device code of qm_boot.inl compiled with -DQM_EMU, on top of the emulated quant object of qm_emu_quant.cpp, which a boot
// object borrows as on the device.  What is here is a C face over the driver's object.  One wavefront after the other, one lane
// after the other: this checks the driver, the draw, the logic of the batched iteration bodies, the order of their sums and the
// per-replicate stop -- not the atomics.
#include "qm_emu_quant.cpp"
#include "../../rapmap_amd/csrc/qm_boot_host.inl"

extern "C" {

// quant: a handle of qe_quant_create.  aggregate: the resample's per-wavefront aggregation on or off (the counts do not depend on it).
void* qe_boot_create(void* quant, int n_reps, int aggregate, int* err) {
  qm_boot* b = new qm_boot();
  b->aggregate = aggregate;
  if ((*err = boot_open(b, (qm_quant*)quant, n_reps))) { delete b; return nullptr; }
  return b;
}
void qe_boot_destroy(void* h) { boot_close((qm_boot*)h); delete (qm_boot*)h; }

// stats: [0] classes [1] entries [2] present [3] N [4] queued labels [5] queued transcripts
void qe_boot_info(void* h, long long* stats) {
  const qm_boot& b = *(qm_boot*)h;
  stats[0] = b.q->nClasses; stats[1] = b.q->nEntries; stats[2] = b.q->present; stats[3] = (long long)b.N; stats[4] = b.nqCls; stats[5] = b.nqTxp;
}
int qe_boot_classes(void* h, long long* off, u32* tids, uint64_t* cnt) { return quant_fetch_classes(((qm_boot*)h)->q, (int64_t*)off, tids, cnt); }
int qe_boot_resample(void* h, u64 seed, long long first_rep) { return boot_resample((qm_boot*)h, seed, first_rep); }
int qe_boot_set_counts(void* h, int rep, const uint64_t* counts) { return boot_set_counts((qm_boot*)h, rep, counts); }
int qe_boot_fetch_counts(void* h, int rep, uint64_t* counts) { return boot_fetch_counts((qm_boot*)h, rep, counts); }
// launches: the class, transcript and mark launches of this run (QM_BOOT_STAT_LAUNCHES)
int qe_boot_run(void* h, int max_iter, int check_every, double rel_tol, double min_alpha, int* iterations, double* last_rel, long long* launches) {
  const int rc = boot_run((qm_boot*)h, max_iter, check_every, rel_tol, min_alpha, iterations, last_rel);
  *launches = ((qm_boot*)h)->lastLaunches;
  return rc;
}
int qe_boot_fetch(void* h, double* out) { return boot_fetch((qm_boot*)h, out); }

void qe_boot_philox(const u32* ctr, const u32* key, u32* out) { boot_philox(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], out); }

}  // extern "C"
