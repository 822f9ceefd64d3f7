// qm_kernels_lean.hip -- the lean stage-A kernel (qm_lean.inl): two reads per wavefront and iteration, for the reads that make up
// nearly all of a batch; what it leaves is mapped by qm_read_kernel (qm_host.hip, run_stage_a)
#include "qm_lean_kernel.inl"

hipError_t qmk_launch_lean(const DevIndex& ix, const ReadBatch& B, int num_cu, hipStream_t st) {
  if (B.lean_wide) return ix.saext2 ? launch_lean<true, false>(ix, B, num_cu, st) : hipErrorInvalidValue;   // reads of 129 .. 256 characters: one per wavefront
  return launch_lean<false, false>(ix, B, num_cu, st);
}
