// qm_lean_kernel.inl -- qm_lean_kernel and its launcher, shared by the compile units that instantiate it (qm_kernels_lean.hip: the first
// pass; qm_kernels_leanq.hip: the N-aware pass over the queue of what the first pass left)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "qm_lean.inl"
#include "qm_device.h"

namespace qm {

template <bool PAIRED, bool SEL, bool PH, bool WIDE = false, bool NQ = false>
__global__ __launch_bounds__(64 * QM_WG_WAVES, 8) void qm_lean_kernel(DevIndex ix_, ReadBatch B_, int rs) {
  const DevIndex& ix = stage_args().ix; const ReadBatch& B = stage_args().B;   // (through the kernarg segment, not ix_ / B_: see stage_args)
  __shared__ __attribute__((aligned(16))) LeanMem mem[QM_WG_WAVES];
  const int wave = QM_WG_WAVES == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  lean_wave<PAIRED, SEL, PH, WIDE, NQ>(ix, B, (int)blockIdx.x * QM_WG_WAVES + wave, (int)gridDim.x * QM_WG_WAVES, mem[wave], rs);
}

}  // namespace qm

using namespace qm;

// One edition (WIDE, NQ) over the batch: the flags of the launch pick the instantiation (lean_dispatch).  B.selscr set: the chain-scoring
// collector of a -s call (intervals and foundHit out, no lists); ix.ph set: the compact -p image.  Grid: qm_grid.h.
template <bool WIDE, bool NQ>
static hipError_t launch_lean(const DevIndex& ix, const ReadBatch& B, int num_cu, hipStream_t st) {
  return lean_dispatch(B.seq2 != nullptr, B.selscr != nullptr, ix.ph != nullptr, [&](auto paired, auto sel, auto ph) {
    constexpr bool PAIRED = decltype(paired)::value, SEL = decltype(sel)::value, PH = decltype(ph)::value;
    const int over = NQ ? 1 : (PH ? grid_oversub_ph() : (SEL ? grid_oversub() : 2 * grid_oversub()));
    const WaveGrid g = wave_grid(lean_iters(B.nreads, WIDE), num_cu, resident_quads_per_cu<qm_lean_kernel<PAIRED, SEL, PH, WIDE, NQ>, 8>("qm_lean_kernel"), over);
    hipLaunchKernelGGL((qm_lean_kernel<PAIRED, SEL, PH, WIDE, NQ>), dim3((unsigned)g.blocks), dim3(64 * QM_WG_WAVES), 0, st, ix, B, g.rs);
    return hipGetLastError();
  });
}
