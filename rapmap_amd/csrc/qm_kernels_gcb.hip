// qm_kernels_gcb.hip -- the kernel of the observed GC sweep (qm_gcb.inl: the one body there that owns an LDS tally) and its launch
// wrapper; the other bodies are plain wave bodies, launched through qm_exec.h where their driver is compiled
#include "qm_gcb.inl"
#include "qm_device.h"

using namespace qm;

#define GCB_BLOCK 256          // four wavefronts, a 128-byte tally each

__global__ void __launch_bounds__(GCB_BLOCK) qm_gcb_obs_kernel(FldSrc S, GcbIdx I, GcbAcc A) {
  __shared__ u32 slab[GCB_BLOCK / 64][GCB_SLAB];
  gcb_obs_wave(S, I, A, uniform(((long long)blockIdx.x * GCB_BLOCK + threadIdx.x) >> 6), (long long)gridDim.x * (GCB_BLOCK / 64), (QM_LDS(u32)*)&slab[threadIdx.x >> 6][0]);
}

hipError_t qmk_gcb_obs(const FldSrc& S, const GcbIdx& I, const GcbAcc& A, int blocks, hipStream_t st) {
  if (S.n <= 0 || blocks <= 0) return hipSuccess;
  hipLaunchKernelGGL(qm_gcb_obs_kernel, dim3((unsigned)blocks), dim3(GCB_BLOCK), 0, st, S, I, A);
  return hipGetLastError();
}
