// qm_kernels_boot.hip -- the kernels of the bootstrap replicates (qm_boot.inl), their launch wrappers, and the rocPRIM scan of the
// snapshot's counts.  A launch with a second grid dimension spreads it over replicate slots (resample, transpose) or over tiles
// of BOOT_TILE replicates (everything replicate-innermost).
#include <hip/hip_runtime.h>
#include <cstring>
#include <type_traits>
#include <cstdlib>
#include <rocprim/rocprim.hpp>

#include "qm_boot.inl"
#include "qm_device.h"

using namespace qm;

#define BOOT_BLOCK 256         // four wavefronts
static inline unsigned boot_blocks(long long waves) { return (unsigned)((waves + BOOT_BLOCK / 64 - 1) / (BOOT_BLOCK / 64)); }
// the wavefront's index along x, wave-uniform by construction; blockIdx.y is uniform as it is
__device__ __forceinline__ long long boot_wave_id() { return uniform(((long long)blockIdx.x * BOOT_BLOCK + threadIdx.x) >> 6); }

__global__ void __launch_bounds__(BOOT_BLOCK) qm_boot_counts_kernel(const double* dcnt, long long nc, u64* out) { boot_counts_wave(dcnt, nc, out, boot_wave_id()); }
__global__ void __launch_bounds__(BOOT_BLOCK) qm_boot_rowflag_kernel(const long long* off, long long n, u32* flag) { boot_rowflag_wave(off, n, flag, boot_wave_id()); }
template <int AGG>
__global__ void __launch_bounds__(BOOT_BLOCK) qm_boot_resample_kernel(BootDraw D, long long waves) {
  const long long w = boot_wave_id();
  D.aggregate = AGG;
  if (w < waves) boot_resample_wave(D, w, (long long)blockIdx.y);
}
__global__ void __launch_bounds__(BOOT_BLOCK) qm_boot_single_kernel(const long long* coff, const u32* clab, long long nc, const u64* cnt, double* single, long long Bp) {
  boot_single_wave(coff, clab, nc, cnt, single, Bp, boot_wave_id(), (long long)blockIdx.y);
}
__global__ void __launch_bounds__(BOOT_BLOCK) qm_boot_column_kernel(const long long* coff, const u32* clab, long long nc, u64* cnt, double* single, long long Bp, long long slot,
                                                                    u64* col, int put) {
  boot_column_wave(coff, clab, nc, cnt, single, Bp, slot, col, put, boot_wave_id());
}
__global__ void __launch_bounds__(BOOT_BLOCK) qm_boot_start_kernel(const long long* toff, const double* eff, long long nTxps, double value, double* alpha, double* w, long long Bp,
                                                                   long long s0, long long ns) {
  boot_start_wave(toff, eff, nTxps, value, alpha, w, Bp, s0, ns, boot_wave_id(), (long long)blockIdx.y);
}
__global__ void __launch_bounds__(BOOT_BLOCK) qm_boot_reset_kernel(BootBook K, long long s0, long long ns) { boot_reset_wave(K, s0, ns, boot_wave_id()); }
__global__ void __launch_bounds__(BOOT_BLOCK) qm_boot_begin_kernel(BootBook K, long long nReps) { boot_begin_wave(K, nReps, boot_wave_id()); }
__global__ void __launch_bounds__(BOOT_BLOCK) qm_boot_mark_kernel(BootBook K, long long nReps, int it, double relTol) { boot_mark_wave(K, nReps, it, relTol, boot_wave_id()); }
__global__ void __launch_bounds__(BOOT_BLOCK) qm_boot_end_kernel(BootBook K, long long nReps, int it) { boot_end_wave(K, nReps, it, boot_wave_id()); }
__global__ void __launch_bounds__(BOOT_BLOCK) qm_boot_transpose_kernel(const double* alpha, long long nTxps, long long Bp, double* out) {
  boot_transpose_wave(alpha, nTxps, Bp, out, boot_wave_id(), (long long)blockIdx.y);
}
// the two launches of an iteration; a wavefront beyond the side's last one (the tail of the last block) has nothing to do
__global__ void __launch_bounds__(BOOT_BLOCK) qm_boot_class_kernel(BootState S, long long waves) {
  const long long w = boot_wave_id();
  if (w < waves) boot_class_wave(S, w, (long long)blockIdx.y);
}
__global__ void __launch_bounds__(BOOT_BLOCK) qm_boot_txp_kernel(BootState S, long long waves) {
  const long long w = boot_wave_id();
  if (w < waves) boot_txp_wave(S, w, (long long)blockIdx.y);
}

extern "C" {
hipError_t qmk_boot_counts(const double* dcnt, long long nc, unsigned long long* out, hipStream_t st) {
  hipLaunchKernelGGL(qm_boot_counts_kernel, dim3(boot_blocks((nc + 1 + 63) / 64)), dim3(BOOT_BLOCK), 0, st, dcnt, nc, (u64*)out);
  return hipGetLastError();
}
hipError_t qmk_boot_rowflag(const long long* off, long long n, unsigned int* flag, hipStream_t st) {
  hipLaunchKernelGGL(qm_boot_rowflag_kernel, dim3(boot_blocks((n + 1 + 63) / 64)), dim3(BOOT_BLOCK), 0, st, off, n, flag);
  return hipGetLastError();
}
// n_slots replicate slots, (N + 1) / 2 Philox calls each
hipError_t qmk_boot_resample(const void* draw, long long n_slots, int aggregate, hipStream_t st) {
  const BootDraw& D = *(const BootDraw*)draw;
  const long long waves = (long long)(((D.N + 1) / 2 + 63) / 64);
  if (waves <= 0 || n_slots <= 0) return hipSuccess;
  if (aggregate) hipLaunchKernelGGL(qm_boot_resample_kernel<1>, dim3(boot_blocks(waves), (unsigned)n_slots), dim3(BOOT_BLOCK), 0, st, D, waves);
  else hipLaunchKernelGGL(qm_boot_resample_kernel<0>, dim3(boot_blocks(waves), (unsigned)n_slots), dim3(BOOT_BLOCK), 0, st, D, waves);
  return hipGetLastError();
}
hipError_t qmk_boot_single(const long long* coff, const unsigned int* clab, long long nc, const unsigned long long* cnt, double* single, long long bp, hipStream_t st) {
  if (nc <= 0) return hipSuccess;
  hipLaunchKernelGGL(qm_boot_single_kernel, dim3(boot_blocks(boot_row_waves(nc)), (unsigned)(bp / BOOT_TILE)), dim3(BOOT_BLOCK), 0, st, coff, clab, nc, (const u64*)cnt, single, bp);
  return hipGetLastError();
}
hipError_t qmk_boot_column(const long long* coff, const unsigned int* clab, long long nc, unsigned long long* cnt, double* single, long long bp, long long slot,
                           unsigned long long* col, int put, hipStream_t st) {
  if (nc <= 0) return hipSuccess;
  hipLaunchKernelGGL(qm_boot_column_kernel, dim3(boot_blocks((nc + 63) / 64)), dim3(BOOT_BLOCK), 0, st, coff, clab, nc, (u64*)cnt, single, bp, slot, (u64*)col, put);
  return hipGetLastError();
}
hipError_t qmk_boot_start(const long long* toff, const double* eff, long long n_txps, double value, double* alpha, double* w, long long bp, long long s0, long long ns, hipStream_t st) {
  if (n_txps <= 0 || ns <= 0) return hipSuccess;
  hipLaunchKernelGGL(qm_boot_start_kernel, dim3(boot_blocks(boot_row_waves(n_txps)), (unsigned)(bp / BOOT_TILE)), dim3(BOOT_BLOCK), 0, st, toff, eff, n_txps, value, alpha, w, bp, s0, ns);
  return hipGetLastError();
}
hipError_t qmk_boot_reset(const void* book, long long s0, long long ns, hipStream_t st) {
  if (ns <= 0) return hipSuccess;
  hipLaunchKernelGGL(qm_boot_reset_kernel, dim3(boot_blocks((ns + 63) / 64)), dim3(BOOT_BLOCK), 0, st, *(const BootBook*)book, s0, ns);
  return hipGetLastError();
}
hipError_t qmk_boot_begin(const void* book, long long n_reps, hipStream_t st) {
  hipLaunchKernelGGL(qm_boot_begin_kernel, dim3(boot_blocks((n_reps + 63) / 64)), dim3(BOOT_BLOCK), 0, st, *(const BootBook*)book, n_reps);
  return hipGetLastError();
}
hipError_t qmk_boot_mark(const void* book, long long n_reps, int it, double rel_tol, hipStream_t st) {
  hipLaunchKernelGGL(qm_boot_mark_kernel, dim3(boot_blocks((n_reps + 63) / 64)), dim3(BOOT_BLOCK), 0, st, *(const BootBook*)book, n_reps, it, rel_tol);
  return hipGetLastError();
}
hipError_t qmk_boot_end(const void* book, long long n_reps, int it, hipStream_t st) {
  hipLaunchKernelGGL(qm_boot_end_kernel, dim3(boot_blocks((n_reps + 63) / 64)), dim3(BOOT_BLOCK), 0, st, *(const BootBook*)book, n_reps, it);
  return hipGetLastError();
}
hipError_t qmk_boot_transpose(const double* alpha, long long n_txps, long long bp, long long n_reps, double* out, hipStream_t st) {
  if (n_txps <= 0 || n_reps <= 0) return hipSuccess;
  hipLaunchKernelGGL(qm_boot_transpose_kernel, dim3(boot_blocks((n_txps + 63) / 64), (unsigned)n_reps), dim3(BOOT_BLOCK), 0, st, alpha, n_txps, bp, out);
  return hipGetLastError();
}
hipError_t qmk_boot_class(const void* state, hipStream_t st) {
  const BootState& S = *(const BootState*)state;
  const long long waves = boot_side_waves(S.cls);
  if (waves <= 0) return hipSuccess;
  hipLaunchKernelGGL(qm_boot_class_kernel, dim3(boot_blocks(waves), (unsigned)(S.Bp / BOOT_TILE)), dim3(BOOT_BLOCK), 0, st, S, waves);
  return hipGetLastError();
}
hipError_t qmk_boot_txp(const void* state, hipStream_t st) {
  const BootState& S = *(const BootState*)state;
  const long long waves = boot_side_waves(S.txp);
  if (waves <= 0) return hipSuccess;
  hipLaunchKernelGGL(qm_boot_txp_kernel, dim3(boot_blocks(waves), (unsigned)(S.Bp / BOOT_TILE)), dim3(BOOT_BLOCK), 0, st, S, waves);
  return hipGetLastError();
}

// exclusive scan of n 64-bit counts (the caller passes one number more than it has classes: the last offset is the total N)
size_t qmk_boot_scan_temp_bytes(long long n) {
  size_t bytes = 0;
  (void)rocprim::exclusive_scan(nullptr, bytes, (const u64*)nullptr, (u64*)nullptr, (u64)0, (size_t)n, rocprim::plus<u64>());
  return bytes;
}
hipError_t qmk_boot_scan(void* temp, size_t temp_bytes, const unsigned long long* in, unsigned long long* out, long long n, hipStream_t st) {
  return rocprim::exclusive_scan(temp, temp_bytes, (const u64*)in, (u64*)out, (u64)0, (size_t)n, rocprim::plus<u64>(), st);
}
}
