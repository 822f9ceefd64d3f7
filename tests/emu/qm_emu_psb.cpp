// tests/emu/qm_emu_psb.cpp -- TEST-ONLY lane emulation of the positional bias model: the driver of rapmap_amd/csrc/qm_psb_host.inl and
// the device code of qm_psb.inl, both compiled with -DQM_EMU (an LV<T> is a 64-entry array, QM_LANES a loop: qm_exec.h), for 256
// compute units.  qm_sqb_host.inl comes first, as in qm_host.hip: the model takes its prefix sums and its weights from there.  What
// is here is a C face over the driver's object; where the library takes the transcripts from a context's replica, the object here
// holds arrays of its own.  One wavefront after the other, one lane after the other: this checks the drivers and the logic of the
// bodies, not the atomics.
#define QM_EMU
#include "../../rapmap_amd/csrc/qm_wave.h"
using namespace qm;
#include "../../rapmap_amd/csrc/qm_sqb_host.inl"
#include "../../rapmap_amd/csrc/qm_psb_host.inl"

struct EmuPsb {
  qm_psb g;
  std::vector<u32> off; std::vector<int> len;
};

extern "C" {

int qe_psb_obs_grid(long long n_units, int max_blocks) { return sweep_grid(n_units, 256, PSB_OBS_BLOCKS_PER_CU, max_blocks); }
int qe_psb_exp_grid(long long n_txps, int max_blocks) { return sweep_grid(n_txps * PSB_POS, 256, PSB_EXP_BLOCKS_PER_CU, max_blocks); }
int qe_psb_tile_grid(long long n_tiles, int max_blocks) { return sweep_grid(n_tiles * 64, 256, SQB_BLOCKS_PER_CU, max_blocks); }

// null: max_len out of range
EmuPsb* qe_psb_create(long long n, long long n_txps, const u32* off, const int* len, int max_len, int max_blocks) {
  if (max_len < 1 || max_len > SQB_MAX_LEN) return nullptr;
  EmuPsb* e = new EmuPsb();
  e->off.assign(off, off + n_txps); e->len.assign(len, len + n_txps);
  e->g.maxLen = max_len; e->g.maxBlocks = max_blocks;
  e->g.lens.assign(len, len + n_txps);
  if (e->g.open("qe_psb_create", 0, 256) || psb_open(&e->g)) { delete e; return nullptr; }
  e->g.I = SqbIdx{nullptr, e->off.data(), e->len.data(), n_txps, n};   // no text: the model never looks at one
  return e;
}
void qe_psb_destroy(EmuPsb* e) { if (e) e->g.close(); delete e; }
// the host arrays in parts of at most max_units units and max_hits hits
int qe_psb_add_hits(EmuPsb* e, long long n, const int64_t* off, const qm_hit* hits, long long max_units, long long max_hits) {
  return psb_add_hits(&e->g, n, off, hits, max_units, max_hits);
}
int qe_psb_add_counts(EmuPsb* e, const uint64_t* obs) { return psb_add_counts(&e->g, obs); }
int qe_psb_clear(EmuPsb* e) { return psb_clear(&e->g); }
// the bins and the SW_C_WORDS counters as they lie in the object's memory
int qe_psb_fetch(EmuPsb* e, u64* bins, u64* ctr) {
  int rc = qx::read(e->g.stream, bins, e->g.d_acc, PSB_BINS * sizeof(u64));
  return rc ? rc : qx::read(e->g.stream, ctr, e->g.d_acc + PSB_BINS, SW_C_WORDS * sizeof(u64));
}
int qe_psb_stat(const EmuPsb* e, int which, int64_t* value) { return psb_stat(&e->g, which, value); }
int qe_psb_expect(EmuPsb* e, const uint64_t* counts, long long n_txps, const uint64_t* q, uint64_t* ex) { return psb_expect(&e->g, counts, n_txps, q, ex); }
int qe_psb_eff_lens(EmuPsb* e, const uint64_t* counts, long long n_txps, const double* R, double* eff) { return psb_eff_lens(&e->g, counts, n_txps, R, eff); }
int qe_psb_position(EmuPsb* e, long long n, const u32* tids, const int* pos, int* out) { return psb_position(&e->g, n, tids, pos, out); }
int qe_psb_weights(int max_len, const uint64_t* counts, long long n_txps, const uint32_t* lens, const double* alpha, uint64_t* q, int32_t* k) {
  return sqb_weights(max_len, counts, n_txps, lens, alpha, q, k);
}
int qe_psb_ratios(const uint64_t* obs, const uint64_t* ex, double* R) { return psb_ratios(obs, ex, R); }

}  // extern "C"
