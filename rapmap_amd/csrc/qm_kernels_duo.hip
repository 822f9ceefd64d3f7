// qm_kernels_duo.hip -- the pair kernel (qm_duo.inl): the two mates of a read pair walked in lockstep by the two halves of one wavefront
// and merged there; what it leaves is mapped by qm_read_kernel and merged by stage B (qm_host.hip, run_stage_a / run_stage_b)
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "qm_duo.inl"
#include "qm_device.h"

namespace qm {

template <bool PH, bool COV>
__global__ __launch_bounds__(64 * QM_WG_WAVES, 8) void qm_duo_kernel(DevIndex ix_, ReadBatch B_, int rs) {
  const DevIndex& ix = stage_args().ix; const ReadBatch& B = stage_args().B;   // (through the kernarg segment, not ix_ / B_: see stage_args)
  __shared__ __attribute__((aligned(16))) DuoMem mem[QM_WG_WAVES];
  const int wave = QM_WG_WAVES == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  duo_wave<PH, COV>(ix, B, (int)blockIdx.x * QM_WG_WAVES + wave, (int)gridDim.x * QM_WG_WAVES, mem[wave], rs);
}

}  // namespace qm

using namespace qm;

// paired reads of up to 128 characters, dense table or (ix.ph set) the compact -p image.  Grid: qm_grid.h.
hipError_t qmk_launch_duo(const DevIndex& ix, const ReadBatch& B, int num_cu, hipStream_t st) {
  if (!B.seq2 || (B.nreads & 1)) return hipErrorInvalidValue;
  static const int knob = [] { const char* e = getenv("QM_DUO_OVERSUB"); return e && atoi(e) > 0 ? atoi(e) : 0; }();
  return duo_dispatch(ix.ph != nullptr, B.quasi_cov > 0.0, [&](auto ph, auto cov) {
    constexpr bool PH = decltype(ph)::value, COV = decltype(cov)::value;
    const int over = knob ? knob : (PH ? grid_oversub_ph() : 2 * grid_oversub());
    const WaveGrid g = wave_grid(pair_iters(B.nreads), num_cu, resident_quads_per_cu<qm_duo_kernel<PH, COV>, 8>("qm_duo_kernel"), over);
    hipLaunchKernelGGL((qm_duo_kernel<PH, COV>), dim3((unsigned)g.blocks), dim3(64 * QM_WG_WAVES), 0, st, ix, B, g.rs);
    return hipGetLastError();
  });
}
