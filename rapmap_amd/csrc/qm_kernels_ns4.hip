// qm_kernels_ns4.hip -- stage-A kernels for reads of up to 256 characters (4 64-character slots per read); see qm_read_kernel.inl
#include "qm_read_kernel.inl"
hipError_t qmk_launch_reads_ns4(const qm::DevIndex& ix, const qm::ReadBatch& B, bool collect, int grid, int num_cu, hipStream_t st) {
  return qm::launch_reads_ns<4, 3, 3, 3, 3, 2, true>(ix, B, collect, grid, num_cu, st);
}
