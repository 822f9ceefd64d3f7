// qm_kernels_fld.hip -- the kernel of the fragment-length histogram (qm_fld.inl) and its launch wrapper
#include "qm_fld.inl"
#include "qm_device.h"

using namespace qm;

#define FLD_BLOCK 256          // four wavefronts, a 4 KB slab each
// workgroups resident per compute unit: 8 waves per SIMD = 32 per CU = 8 workgroups (16 KB of LDS each: 128 of the CU's 160 KB)
#define FLD_BLOCKS_PER_CU 8

__global__ void __launch_bounds__(FLD_BLOCK) qm_fld_fold_kernel(FldSrc S, FldAcc A) {
  __shared__ u32 slab[FLD_BLOCK / 64][FLD_SLAB];
  fld_wave(S, A, uniform(((long long)blockIdx.x * FLD_BLOCK + threadIdx.x) >> 6), (long long)gridDim.x * (FLD_BLOCK / 64), (QM_LDS(u32)*)&slab[threadIdx.x >> 6][0]);
}

extern "C" {
// a persistent grid: the workgroups that are resident at once, fewer when the units do not fill them, at most max_blocks when given
int qmk_fld_grid(long long n_units, int num_cu, int max_blocks) {
  long long g = (long long)(num_cu > 0 ? num_cu : 1) * FLD_BLOCKS_PER_CU;
  const long long need = (n_units + FLD_BLOCK - 1) / FLD_BLOCK;
  if (g > need) g = need;
  if (max_blocks > 0 && g > max_blocks) g = max_blocks;
  return g < 1 ? 1 : (int)g;
}
hipError_t qmk_fld_fold(const void* src, const void* acc, int blocks, hipStream_t st) {
  const FldSrc& S = *(const FldSrc*)src;
  if (S.n <= 0 || blocks <= 0) return hipSuccess;
  hipLaunchKernelGGL(qm_fld_fold_kernel, dim3((unsigned)blocks), dim3(FLD_BLOCK), 0, st, S, *(const FldAcc*)acc);
  return hipGetLastError();
}
}
