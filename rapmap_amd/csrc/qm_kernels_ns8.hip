// qm_kernels_ns8.hip -- stage-A kernels for reads of up to 512 characters (8 64-character slots per read); see qm_read_kernel.inl
#include "qm_read_kernel.inl"
hipError_t qmk_launch_reads_ns8(const qm::DevIndex& ix, const qm::ReadBatch& B, bool collect, int grid, int num_cu, hipStream_t st) {
  return qm::launch_reads_ns<8, 2, 2, 2, 2, 1, true>(ix, B, collect, grid, num_cu, st);
}
