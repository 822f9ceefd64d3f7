// tests/emu/qm_emu_sqb.cpp -- TEST-ONLY lane emulation of the sequence-specific bias model: the driver of rapmap_amd/csrc/qm_sqb_host.inl
// and the device code of qm_sqb.inl, both compiled with -DQM_EMU (an LV<T> is a 64-entry array, QM_LANES a loop: qm_exec.h), for 256
// compute units.  What is here is a C face over the driver's object; where the library takes text and transcripts from a context's
// replica, the object here holds arrays of its own.  One wavefront after the other, one lane after the other: this checks the
// drivers and the logic of the bodies, not the atomics.
#define QM_EMU
#include "../../rapmap_amd/csrc/qm_wave.h"
using namespace qm;
#include "../../rapmap_amd/csrc/qm_sqb_host.inl"

struct EmuSqb {
  qm_sqb g;
  std::vector<unsigned char> text; std::vector<u32> off; std::vector<int> len;
};

extern "C" {

int qe_sqb_obs_grid(long long n_units, int max_blocks) { return sweep_grid(n_units, 256, SQB_OBS_BLOCKS_PER_CU, max_blocks); }
int qe_sqb_tile_grid(long long n_tiles, int max_blocks) { return sweep_grid(n_tiles * 64, 256, SQB_BLOCKS_PER_CU, max_blocks); }

// null: max_len out of range
EmuSqb* qe_sqb_create(const unsigned char* text, long long n, long long n_txps, const u32* off, const int* len, int max_len, int max_blocks) {
  if (max_len < 1 || max_len > SQB_MAX_LEN) return nullptr;
  EmuSqb* e = new EmuSqb();
  e->text.assign(text, text + n); e->off.assign(off, off + n_txps); e->len.assign(len, len + n_txps);
  e->g.maxLen = max_len; e->g.maxBlocks = max_blocks;
  e->g.lens.assign(len, len + n_txps);
  if (e->g.open("qe_sqb_create", 0, 256) || sqb_open(&e->g)) { delete e; return nullptr; }
  e->g.I = SqbIdx{e->text.data(), e->off.data(), e->len.data(), n_txps, n};
  return e;
}
void qe_sqb_destroy(EmuSqb* e) { if (e) e->g.close(); delete e; }
// the host arrays in parts of at most max_units units and max_hits hits
int qe_sqb_add_hits(EmuSqb* e, long long n, const int64_t* off, const qm_hit* hits, long long max_units, long long max_hits) {
  return sqb_add_hits(&e->g, n, off, hits, max_units, max_hits);
}
int qe_sqb_add_counts(EmuSqb* e, const uint64_t* obs) { return sqb_add_counts(&e->g, obs); }
int qe_sqb_clear(EmuSqb* e) { return sqb_clear(&e->g); }
// the bins and the SW_C_WORDS counters as they lie in the object's memory
int qe_sqb_fetch(EmuSqb* e, u64* bins, u64* ctr) {
  int rc = qx::read(e->g.stream, bins, e->g.d_acc, SQB_BINS * sizeof(u64));
  return rc ? rc : qx::read(e->g.stream, ctr, e->g.d_acc + SQB_BINS, SW_C_WORDS * sizeof(u64));
}
int qe_sqb_stat(const EmuSqb* e, int which, int64_t* value) { return sqb_stat(&e->g, which, value); }
int qe_sqb_expect(EmuSqb* e, const uint64_t* counts, long long n_txps, const uint64_t* q, uint64_t* ex) { return sqb_expect(&e->g, counts, n_txps, q, ex); }
int qe_sqb_eff_lens(EmuSqb* e, const uint64_t* counts, long long n_txps, const double* R, double* eff) { return sqb_eff_lens(&e->g, counts, n_txps, R, eff); }
int qe_sqb_context(EmuSqb* e, long long n, const u32* tids, const int* pos, const int* ends, int* out) { return sqb_context(&e->g, n, tids, pos, ends, out); }
int qe_sqb_weights(int max_len, const uint64_t* counts, long long n_txps, const uint32_t* lens, const double* alpha, uint64_t* q, int32_t* k) {
  return sqb_weights(max_len, counts, n_txps, lens, alpha, q, k);
}
int qe_sqb_ratios(const uint64_t* obs, const uint64_t* ex, double* R) { return sqb_ratios(obs, ex, R); }

}  // extern "C"
