// qm_kernels_eqc.hip -- the kernels of the equivalence-class table that are no plain wave body (an LDS slab per wavefront, one
// thread per entry, a grid-stride sum) and their launch wrappers; the wave bodies of qm_eqc.inl are launched by qm_eqc_host.inl
// through qm_exec.h
#include "qm_eqc.inl"
#include "qm_device.h"

using namespace qm;

#define EQC_BLOCK 256          // four wavefronts
static inline unsigned eqc_blocks(long long waves) { return (unsigned)((waves + EQC_BLOCK / 64 - 1) / (EQC_BLOCK / 64)); }
__device__ __forceinline__ long long eqc_wave_id() { return ((long long)blockIdx.x * EQC_BLOCK + threadIdx.x) >> 6; }

__global__ void __launch_bounds__(EQC_BLOCK) qm_eqc_label_queued_kernel(EqcSrc S, long long nq) {
  __shared__ u32 slab[EQC_BLOCK / 64][EQC_SLAB];
  const long long w = eqc_wave_id();
  if (w < nq) eqc_label_queued(S, w, (QM_LDS(u32)*)&slab[threadIdx.x >> 6][0]);
}
// after the table has grown every pending unit starts its probe sequence anew
__global__ void __launch_bounds__(EQC_BLOCK) qm_eqc_reset_probes_kernel(u64* q, long long n) {
  const long long i = (long long)blockIdx.x * EQC_BLOCK + threadIdx.x;
  if (i < n) q[i] &= 0xffffffffULL;
}
__global__ void __launch_bounds__(EQC_BLOCK) qm_eqc_sum_kernel(const u64* count, const u64* key, long long cap, u64* out) {
  u64 s = 0;
  for (long long i = (long long)blockIdx.x * EQC_BLOCK + threadIdx.x; i < cap; i += (long long)gridDim.x * EQC_BLOCK) if (key[i]) s += count[i];
  if (s) atomicAdd(out, s);
}

hipError_t qmk_eqc_label_queued(const EqcSrc& S, long long nq, hipStream_t st) {
  if (nq <= 0) return hipSuccess;
  hipLaunchKernelGGL(qm_eqc_label_queued_kernel, dim3(eqc_blocks(nq)), dim3(EQC_BLOCK), 0, st, S, nq);
  return hipGetLastError();
}
hipError_t qmk_eqc_reset_probes(unsigned long long* q, long long n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(qm_eqc_reset_probes_kernel, dim3((unsigned)((n + EQC_BLOCK - 1) / EQC_BLOCK)), dim3(EQC_BLOCK), 0, st, (u64*)q, n);
  return hipGetLastError();
}
hipError_t qmk_eqc_sum(const unsigned long long* count, const unsigned long long* key, long long cap, unsigned long long* out, hipStream_t st) {
  if (cap <= 0) return hipSuccess;
  long long blocks = (cap + EQC_BLOCK - 1) / EQC_BLOCK; if (blocks > 256) blocks = 256;
  hipLaunchKernelGGL(qm_eqc_sum_kernel, dim3((unsigned)blocks), dim3(EQC_BLOCK), 0, st, (const u64*)count, (const u64*)key, cap, (u64*)out);
  return hipGetLastError();
}
