// qm_kernels_ns3.hip -- stage-A kernels for reads of up to 192 characters (3 64-character slots per read); see qm_read_kernel.inl
#include "qm_read_kernel.inl"
hipError_t qmk_launch_reads_ns3(const qm::DevIndex& ix, const qm::ReadBatch& B, bool collect, int grid, int num_cu, hipStream_t st) {
  return qm::launch_reads_ns<3, 6, 5, 6, 5, 3, true, 8>(ix, B, collect, grid, num_cu, st);
}
