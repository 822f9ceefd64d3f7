// qm_kernels_lib.hip -- the two persistent kernels of the library-type sweep (qm_lib.inl) and their launch wrappers; the compaction
// is a plain wave body and is launched through qm_exec.h where the driver is (qm_lib_host.inl)
#include "qm_lib.inl"
#include "qm_device.h"

using namespace qm;

#define LIB_BLOCK 256          // four wavefronts, no LDS
// workgroups resident per compute unit: 8 waves per SIMD = 32 per CU = 8 workgroups
#define LIB_BLOCKS_PER_CU 8

__global__ void __launch_bounds__(LIB_BLOCK) qm_lib_classify_kernel(LibSrc S, LibAcc A) {
  lib_classify_wave(S, A, uniform(((long long)blockIdx.x * LIB_BLOCK + threadIdx.x) >> 6), (long long)gridDim.x * (LIB_BLOCK / 64));
}
__global__ void __launch_bounds__(LIB_BLOCK) qm_lib_units_kernel(LibSrc S, LibAcc A) {
  lib_units_wave(S, A, uniform(((long long)blockIdx.x * LIB_BLOCK + threadIdx.x) >> 6), (long long)gridDim.x * (LIB_BLOCK / 64));
}

extern "C" {
// a persistent grid over `lanes` hits or units (qm_grid.h): the workgroups that are resident at once, fewer when the work does not
// fill them, at most max_blocks when given
int qmk_lib_grid(long long lanes, int num_cu, int max_blocks) {
  const int g = grid_blocks((lanes + 63) / 64, num_cu > 0 ? num_cu : 1, LIB_BLOCKS_PER_CU, 1);
  return max_blocks > 0 && g > max_blocks ? max_blocks : g;
}
hipError_t qmk_lib_classify(const void* src, const void* acc, int blocks, hipStream_t st) {
  const LibSrc& S = *(const LibSrc*)src;
  if (S.nh <= 0 || blocks <= 0) return hipSuccess;
  hipLaunchKernelGGL(qm_lib_classify_kernel, dim3((unsigned)blocks), dim3(LIB_BLOCK), 0, st, S, *(const LibAcc*)acc);
  return hipGetLastError();
}
hipError_t qmk_lib_units(const void* src, const void* acc, int blocks, hipStream_t st) {
  const LibSrc& S = *(const LibSrc*)src;
  if (S.n <= 0 || blocks <= 0) return hipSuccess;
  hipLaunchKernelGGL(qm_lib_units_kernel, dim3((unsigned)blocks), dim3(LIB_BLOCK), 0, st, S, *(const LibAcc*)acc);
  return hipGetLastError();
}
}
