// tests/emu/qm_emu_fld.cpp -- TEST-ONLY lane emulation of the fragment-length sweep: rapmap_amd/csrc/qm_fld.inl compiled with
// -DQM_EMU (an LV<T> is a 64-entry array, QM_LANES a loop), driven the way qm_fld_host.inl drives the kernel: a persistent grid of
// four wavefronts per workgroup, capped when the caller says so.  One wavefront after the other, one lane after the other: this
// checks the logic of the sweep -- offsets, categories, the slab, the flush --, not the atomics.  Every wavefront's slab is handed
// over filled with 0xA5: the body must zero what it uses.
#define QM_EMU
#include "../../rapmap_amd/csrc/qm_fld.inl"

#include <vector>

using namespace qm;

extern "C" {

// the grid of qmk_fld_grid (qm_kernels_fld.hip) for 256 compute units: workgroups of 256 threads, eight resident per unit
int qe_fld_grid(long long n_units, int max_blocks) {
  long long g = 256LL * 8;
  const long long need = (n_units + 255) / 256;
  if (g > need) g = need;
  if (max_blocks > 0 && g > max_blocks) g = max_blocks;
  return g < 1 ? 1 : (int)g;
}

// folds n units into bins[FLD_SLAB] / ctr[FLD_C_WORDS] (added to, not cleared); hits may be null when no unit has a hit
int qe_fld_fold(long long n, const long long* off, const unsigned char* hits, int stride, int max_len, int max_blocks, u64* bins, u64* ctr) {
  if (max_len < 1 || max_len > FLD_SLAB - 1) return -1;
  if (n <= 0) return 0;
  const FldSrc S{hits, stride, off, n};
  const FldAcc A{bins, ctr, max_len};
  const long long waves = 4LL * qe_fld_grid(n, max_blocks);
  std::vector<u32> slab(FLD_SLAB);
  for (long long w = 0; w < waves; ++w) {
    slab.assign(FLD_SLAB, 0xA5A5A5A5u);
    fld_wave(S, A, w, waves, slab.data());
  }
  return 0;
}

}  // extern "C"
