// tests/emu/qm_emu_gcb.cpp -- TEST-ONLY lane emulation of the fragment GC bias model: the driver of rapmap_amd/csrc/qm_gcb_host.inl
// and the device code of qm_gcb.inl, both compiled with -DQM_EMU (an LV<T> is a 64-entry array, QM_LANES a loop: qm_exec.h), for 256
// compute units.  What is here is a C face over the driver's object; where the library takes text and transcripts from a context's
// replica, the object here holds arrays of its own and builds the rank structure from them with the driver's own function.  One
// wavefront after the other, one lane after the other: this checks the drivers and the logic of the bodies, not the atomics.
#define QM_EMU
#include "../../rapmap_amd/csrc/qm_wave.h"
using namespace qm;
#include "../../rapmap_amd/csrc/qm_gcb_host.inl"

struct EmuGcb {
  qm_gcb g;
  std::vector<unsigned char> text; std::vector<u32> off; std::vector<int> len;
  DevBuf<u64> mask; DevBuf<u32> rank; DevBuf<unsigned char> tmp;
};

extern "C" {

int qe_gcb_obs_grid(long long n_units, int max_blocks) { return sweep_grid(n_units, 256, GCB_BLOCKS_PER_CU, max_blocks); }

// null: max_len out of range
EmuGcb* qe_gcb_create(const unsigned char* text, long long n, long long n_txps, const u32* off, const int* len, int max_len, int max_blocks) {
  if (max_len < 1 || max_len > GCB_MAX_LEN) return nullptr;
  EmuGcb* e = new EmuGcb();
  e->text.assign(text, text + n); e->off.assign(off, off + n_txps); e->len.assign(len, len + n_txps);
  e->g.maxLen = max_len; e->g.maxBlocks = max_blocks;
  for (long long t = 0; t < n_txps; ++t) e->g.maxTxpLen = std::max<long long>(e->g.maxTxpLen, len[t]);
  if (e->g.open("qe_gcb_create", 0, 256) || gcb_open(&e->g) || gcb_build_rank(e->g.stream, e->text.data(), n, e->mask, e->rank, e->tmp)) { delete e; return nullptr; }
  e->g.I = GcbIdx{e->mask, e->rank, e->off.data(), e->len.data(), n_txps, n};
  return e;
}
void qe_gcb_destroy(EmuGcb* e) { if (e) e->g.close(); delete e; }
// the rank structure as built: gcb_blocks(n) masks and ranks
long long qe_gcb_rank(EmuGcb* e, u64* mask, u32* rank) {
  const long long nb = gcb_blocks(e->g.I.n);
  if (mask) { memcpy(mask, e->mask.p, (size_t)nb * 8); memcpy(rank, e->rank.p, (size_t)nb * 4); }
  return nb;
}
// the host arrays in parts of at most max_units units and max_hits hits
int qe_gcb_add_hits(EmuGcb* e, long long n, const int64_t* off, const qm_hit* hits, long long max_units, long long max_hits) {
  return gcb_add_hits(&e->g, n, off, hits, max_units, max_hits);
}
int qe_gcb_add_counts(EmuGcb* e, const uint64_t* obs) { return gcb_add_counts(&e->g, obs); }
int qe_gcb_clear(EmuGcb* e) { return gcb_clear(&e->g); }
// the WHOLE slab (GCB_SLAB words, not only the bins) and the GCB_C_WORDS counters as they lie in the object's memory
int qe_gcb_fetch(EmuGcb* e, u64* slab, u64* ctr) {
  int rc = qx::read(e->g.stream, slab, e->g.d_acc, GCB_SLAB * sizeof(u64));
  return rc ? rc : qx::read(e->g.stream, ctr, e->g.d_acc + GCB_SLAB, GCB_C_WORDS * sizeof(u64));
}
int qe_gcb_stat(const EmuGcb* e, int which, int64_t* value) { return gcb_stat(&e->g, which, value); }
int qe_gcb_expect(EmuGcb* e, const uint64_t* counts, long long n_txps, uint64_t* H) { return gcb_expect(&e->g, counts, n_txps, H); }
int qe_gcb_window_gc(EmuGcb* e, long long n, const u32* tids, const int* starts, const int* lens, int* out) { return gcb_window_gc(&e->g, n, tids, starts, lens, out); }

}  // extern "C"
