// qm_kernels_quant.hip -- the kernels of the EM over the equivalence-class table (qm_quant.inl), their launch wrappers, and the
// rocPRIM calls of the structure build (two kinds of exclusive scan, one stable sort of (tid, class) pairs)
#include <hip/hip_runtime.h>
#include <cstring>
#include <type_traits>
#include <cstdlib>
#include <rocprim/rocprim.hpp>

#include "qm_quant.inl"
#include "qm_device.h"

using namespace qm;

#define QNT_BLOCK 256          // four wavefronts
static inline unsigned qnt_blocks(long long waves) { return (unsigned)((waves + QNT_BLOCK / 64 - 1) / (QNT_BLOCK / 64)); }
// the wavefront's index in the launch, wave-uniform by construction: what is decided from it is decided on the scalar unit
__device__ __forceinline__ long long qnt_wave_id() { return uniform(((long long)blockIdx.x * QNT_BLOCK + threadIdx.x) >> 6); }

__global__ void __launch_bounds__(QNT_BLOCK) qm_quant_mark_kernel(QuantBuild B) { quant_mark_wave(B, qnt_wave_id()); }
__global__ void __launch_bounds__(QNT_BLOCK) qm_quant_compact_kernel(QuantBuild B) { quant_compact_wave(B, qnt_wave_id()); }
__global__ void __launch_bounds__(QNT_BLOCK) qm_quant_bounds_kernel(const u32* sortedTid, long long n, long long nTxps, long long* bound) {
  quant_bounds_wave(sortedTid, n, nTxps, bound, qnt_wave_id());
}
__global__ void __launch_bounds__(QNT_BLOCK) qm_quant_rowstat_kernel(const long long* off, long long n, u32* flag, u64* scal, int maxWord, int present) {
  quant_rowstat_wave(off, n, flag, scal, maxWord, present, qnt_wave_id());
}
__global__ void __launch_bounds__(QNT_BLOCK) qm_quant_queue_kernel(const u32* flag, const long long* pos, long long n, long long* queue) {
  quant_queue_wave(flag, pos, n, queue, qnt_wave_id());
}
__global__ void __launch_bounds__(QNT_BLOCK) qm_quant_start_kernel(const long long* toff, long long nTxps, double value, double* alpha) {
  quant_start_wave(toff, nTxps, value, alpha, qnt_wave_id());
}
__global__ void __launch_bounds__(QNT_BLOCK) qm_quant_weights_kernel(const double* alpha, const double* eff, long long nTxps, double* w) {
  quant_weights_wave(alpha, eff, nTxps, w, qnt_wave_id());
}
// the two launches of an iteration; a wavefront beyond the side's last one (the tail of the last block) has nothing to do
__global__ void __launch_bounds__(QNT_BLOCK) qm_quant_class_kernel(QuantState Q, long long waves) {
  const long long w = qnt_wave_id();
  if (w < waves) quant_class_wave(Q, w);
}
__global__ void __launch_bounds__(QNT_BLOCK) qm_quant_txp_kernel(QuantState Q, long long waves) {
  const long long w = qnt_wave_id();
  if (w < waves) quant_txp_wave(Q, w);
}

namespace {
struct QntU32ToI64 { __device__ __host__ long long operator()(u32 x) const { return (long long)x; } };
}

extern "C" {
hipError_t qmk_quant_mark(const void* build, hipStream_t st) {
  const QuantBuild& B = *(const QuantBuild*)build;
  hipLaunchKernelGGL(qm_quant_mark_kernel, dim3(qnt_blocks((B.cap + 1 + 63) / 64)), dim3(QNT_BLOCK), 0, st, B);
  return hipGetLastError();
}
hipError_t qmk_quant_compact(const void* build, hipStream_t st) {
  const QuantBuild& B = *(const QuantBuild*)build;
  hipLaunchKernelGGL(qm_quant_compact_kernel, dim3(qnt_blocks((B.cap + 1 + 63) / 64)), dim3(QNT_BLOCK), 0, st, B);
  return hipGetLastError();
}
hipError_t qmk_quant_bounds(const unsigned int* sorted_tid, long long n, long long n_txps, long long* bound, hipStream_t st) {
  hipLaunchKernelGGL(qm_quant_bounds_kernel, dim3(qnt_blocks((n_txps + 1 + 63) / 64)), dim3(QNT_BLOCK), 0, st, sorted_tid, n, n_txps, bound);
  return hipGetLastError();
}
hipError_t qmk_quant_rowstat(const long long* off, long long n, unsigned int* flag, unsigned long long* scal, int max_word, int present, hipStream_t st) {
  hipLaunchKernelGGL(qm_quant_rowstat_kernel, dim3(qnt_blocks((n + 1 + 63) / 64)), dim3(QNT_BLOCK), 0, st, off, n, flag, (u64*)scal, max_word, present);
  return hipGetLastError();
}
hipError_t qmk_quant_queue(const unsigned int* flag, const long long* pos, long long n, long long* queue, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(qm_quant_queue_kernel, dim3(qnt_blocks((n + 63) / 64)), dim3(QNT_BLOCK), 0, st, flag, pos, n, queue);
  return hipGetLastError();
}
hipError_t qmk_quant_start(const long long* toff, long long n_txps, double value, double* alpha, hipStream_t st) {
  if (n_txps <= 0) return hipSuccess;
  hipLaunchKernelGGL(qm_quant_start_kernel, dim3(qnt_blocks((n_txps + 63) / 64)), dim3(QNT_BLOCK), 0, st, toff, n_txps, value, alpha);
  return hipGetLastError();
}
hipError_t qmk_quant_weights(const double* alpha, const double* eff, long long n_txps, double* w, hipStream_t st) {
  if (n_txps <= 0) return hipSuccess;
  hipLaunchKernelGGL(qm_quant_weights_kernel, dim3(qnt_blocks((n_txps + 63) / 64)), dim3(QNT_BLOCK), 0, st, alpha, eff, n_txps, w);
  return hipGetLastError();
}
hipError_t qmk_quant_class(const void* state, hipStream_t st) {
  const QuantState& Q = *(const QuantState*)state;
  const long long waves = quant_side_waves(Q.cls);
  if (waves <= 0) return hipSuccess;
  hipLaunchKernelGGL(qm_quant_class_kernel, dim3(qnt_blocks(waves)), dim3(QNT_BLOCK), 0, st, Q, waves);
  return hipGetLastError();
}
hipError_t qmk_quant_txp(const void* state, hipStream_t st) {
  const QuantState& Q = *(const QuantState*)state;
  const long long waves = quant_side_waves(Q.txp);
  if (waves <= 0) return hipSuccess;
  hipLaunchKernelGGL(qm_quant_txp_kernel, dim3(qnt_blocks(waves)), dim3(QNT_BLOCK), 0, st, Q, waves);
  return hipGetLastError();
}

// exclusive scan of n 32-bit numbers into 64-bit offsets (the caller passes one number more than it has: the last offset is the total)
size_t qmk_quant_scan_temp_bytes(long long n) {
  size_t bytes = 0;
  auto it = rocprim::make_transform_iterator((const u32*)nullptr, QntU32ToI64());
  (void)rocprim::exclusive_scan(nullptr, bytes, it, (long long*)nullptr, 0LL, (size_t)n, rocprim::plus<long long>());
  return bytes;
}
hipError_t qmk_quant_scan(void* temp, size_t temp_bytes, const unsigned int* in, long long* out, long long n, hipStream_t st) {
  auto it = rocprim::make_transform_iterator(in, QntU32ToI64());
  return rocprim::exclusive_scan(temp, temp_bytes, it, out, 0LL, (size_t)n, rocprim::plus<long long>(), st);
}
// stable sort of n (tid, class) pairs by tid: pairs emitted in class order leave every transcript's classes ascending
size_t qmk_quant_sort_temp_bytes(long long n) {
  size_t bytes = 0;
  (void)rocprim::radix_sort_pairs(nullptr, bytes, (const u32*)nullptr, (u32*)nullptr, (const u32*)nullptr, (u32*)nullptr, (size_t)n);
  return bytes;
}
hipError_t qmk_quant_sort(void* temp, size_t temp_bytes, const unsigned int* tid_in, unsigned int* tid_out, const unsigned int* cls_in, unsigned int* cls_out,
                          long long n, hipStream_t st) {
  return rocprim::radix_sort_pairs(temp, temp_bytes, tid_in, tid_out, cls_in, cls_out, (size_t)n, 0, 32, st);
}
}
