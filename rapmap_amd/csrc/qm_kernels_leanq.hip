// qm_kernels_leanq.hip -- qm_lean_kernel's N-aware edition (lean_iter<..., NQ>): the second pass of stage A over the queue of the reads the
// first pass left, when enough of them are there because of an N (qm_host.hip, run_stage_a)
#include "qm_lean_kernel.inl"

using namespace qm;

// The N-aware edition over a queue (B.slowq[0 .. B.nreads): reads of the batch the first pass left): reads whose characters outside A C G T
// are all N are mapped here, the others marked again (qm_host.hip, run_stage_a).  Not for the wide edition.
hipError_t qmk_launch_lean_nq(const DevIndex& ix, const ReadBatch& B, int num_cu, hipStream_t st) {
  if (B.lean_wide || !B.slowq) return hipErrorInvalidValue;
  return launch_lean<false, true>(ix, B, num_cu, st);
}
