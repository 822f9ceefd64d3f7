// qm_kernels_fld.hip -- the kernel of the fragment-length histogram (qm_fld.inl) and its launch wrapper
#include "qm_fld.inl"
#include "qm_device.h"

using namespace qm;

#define FLD_BLOCK 256          // four wavefronts, a 4 KB slab each

__global__ void __launch_bounds__(FLD_BLOCK) qm_fld_fold_kernel(FldSrc S, FldAcc A) {
  __shared__ u32 slab[FLD_BLOCK / 64][FLD_SLAB];
  fld_wave(S, A, uniform(((long long)blockIdx.x * FLD_BLOCK + threadIdx.x) >> 6), (long long)gridDim.x * (FLD_BLOCK / 64), (QM_LDS(u32)*)&slab[threadIdx.x >> 6][0]);
}

hipError_t qmk_fld_fold(const FldSrc& S, const FldAcc& A, int blocks, hipStream_t st) {
  if (S.n <= 0 || blocks <= 0) return hipSuccess;
  hipLaunchKernelGGL(qm_fld_fold_kernel, dim3((unsigned)blocks), dim3(FLD_BLOCK), 0, st, S, A);
  return hipGetLastError();
}
