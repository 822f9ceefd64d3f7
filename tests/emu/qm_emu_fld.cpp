// tests/emu/qm_emu_fld.cpp -- TEST-ONLY lane emulation of the fragment-length histogram: the driver of rapmap_amd/csrc/qm_fld_host.inl
// and the device code of qm_fld.inl, both compiled with -DQM_EMU (an LV<T> is a 64-entry array, QM_LANES a loop: qm_exec.h), for 256
// compute units.  What is here is a C face over the driver's object.  One wavefront after the other, one lane after the other, each on
// a slab filled with 0xA5 (qx::sweep's emulation, qm_exec.h): this checks the driver and the logic of the sweep -- the parts of host
// arrays, offsets, categories, the slab, the flush, the grid's cap --, not the atomics.
#define QM_EMU
#include "../../rapmap_amd/csrc/qm_wave.h"
using namespace qm;
#include "../../rapmap_amd/csrc/qm_fld_host.inl"

extern "C" {

int qe_fld_grid(long long n_units, int max_blocks) { return sweep_grid(n_units, 256, FLD_BLOCKS_PER_CU, max_blocks); }

// null: max_len out of range
qm_fld* qe_fld_create(int max_len, int max_blocks) {
  if (max_len < 1 || max_len > FLD_SLAB - 1) return nullptr;
  qm_fld* f = new qm_fld();
  f->maxLen = max_len; f->maxBlocks = max_blocks;
  if (f->open("qe_fld_create", 0, 256) || fld_open(f)) { delete f; return nullptr; }
  return f;
}
void qe_fld_destroy(qm_fld* f) { if (f) f->close(); delete f; }
// the host arrays in parts of at most max_units units and max_hits hits
int qe_fld_add_hits(qm_fld* f, long long n, const int64_t* off, const qm_hit* hits, long long max_units, long long max_hits) {
  return fld_add_hits(f, n, off, hits, max_units, max_hits);
}
int qe_fld_add_counts(qm_fld* f, const uint64_t* counts) { return fld_add_counts(f, counts); }
int qe_fld_clear(qm_fld* f) { return fld_clear(f); }
// the WHOLE slab (FLD_SLAB words, not only max_len + 1) and the FLD_C_WORDS counters as they lie in the object's memory
int qe_fld_fetch(qm_fld* f, u64* slab, u64* ctr) {
  int rc = qx::read(f->stream, slab, f->d_acc, FLD_SLAB * sizeof(u64));
  return rc ? rc : qx::read(f->stream, ctr, f->d_acc + FLD_SLAB, FLD_C_WORDS * sizeof(u64));
}
int qe_fld_stat(const qm_fld* f, int which, int64_t* value) { return fld_stat(f, which, value); }

}  // extern "C"
