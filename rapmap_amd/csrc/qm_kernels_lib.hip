// qm_kernels_lib.hip -- the two persistent kernels of the library-type sweep (qm_lib.inl) and their launch wrappers; the compaction
// is a plain wave body and is launched through qm_exec.h where the driver is (qm_lib_host.inl)
#include "qm_lib.inl"
#include "qm_device.h"

using namespace qm;

#define LIB_BLOCK 256          // four wavefronts, no LDS

__global__ void __launch_bounds__(LIB_BLOCK) qm_lib_classify_kernel(LibSrc S, LibAcc A) {
  lib_classify_wave(S, A, uniform(((long long)blockIdx.x * LIB_BLOCK + threadIdx.x) >> 6), (long long)gridDim.x * (LIB_BLOCK / 64));
}
__global__ void __launch_bounds__(LIB_BLOCK) qm_lib_units_kernel(LibSrc S, LibAcc A) {
  lib_units_wave(S, A, uniform(((long long)blockIdx.x * LIB_BLOCK + threadIdx.x) >> 6), (long long)gridDim.x * (LIB_BLOCK / 64));
}

hipError_t qmk_lib_classify(const LibSrc& S, const LibAcc& A, int blocks, hipStream_t st) {
  if (S.nh <= 0 || blocks <= 0) return hipSuccess;
  hipLaunchKernelGGL(qm_lib_classify_kernel, dim3((unsigned)blocks), dim3(LIB_BLOCK), 0, st, S, A);
  return hipGetLastError();
}
hipError_t qmk_lib_units(const LibSrc& S, const LibAcc& A, int blocks, hipStream_t st) {
  if (S.n <= 0 || blocks <= 0) return hipSuccess;
  hipLaunchKernelGGL(qm_lib_units_kernel, dim3((unsigned)blocks), dim3(LIB_BLOCK), 0, st, S, A);
  return hipGetLastError();
}
