// qm_exec.h -- what the drivers of the estimation objects (qm_eqc_host.inl, qm_quant_host.inl, qm_boot_host.inl) run on: a buffer
// type, the launch of a wave body over a number of wavefronts, two scans and a sort, and five host operations.  Like qm_wave.h it
// has two definitions.  In the library (included by qm_host.hip, after DevBuf, PinBuf, fail and HIPCHK) a launch is a kernel on a
// stream, the scans and the sort are rocPRIM's, and the host operations are HIP's.  With -DQM_EMU (tests/emu only) a buffer is a
// vector, a launch is a loop over the wavefronts, one after the other, and the rest is serial host code: the drivers are the same
// text in both builds, so the CPU suite runs the drivers and not a transcription of them.
// A kernel that is not a plain wave body (an LDS slab per wavefront, a persistent grid) is not launched through here: it keeps its
// own kernel and a named launch function with two definitions next to its driver.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>
#include "qm_wave.h"

#ifdef QM_EMU
#include <numeric>
#include "../../include/qmap_mi355.h"

static int fail(int code, const char*, ...) { return code; }
#define HIPCHK(x) do { if ((x) != 0) return fail(QM_E_NOGPU, #x); } while (0)

template <typename T>
struct DevBuf {
  std::vector<T> v; T* p = nullptr; int64_t cap = 0;
  operator T*() const { return p; }
  void swap(DevBuf& o) { v.swap(o.v); std::swap(p, o.p); std::swap(cap, o.cap); }
  int ensure(int64_t want) {
    if (want <= cap && p) return QM_OK;
    v.assign((size_t)want, T()); p = v.data(); cap = want;
    return QM_OK;
  }
};
template <typename T> using PinBuf = DevBuf<T>;
#else
#include <rocprim/rocprim.hpp>
#endif

// (the layer's own functions answer with a QM_* code, a launch with what HIPCHK takes)
#define QXCHK(x) do { if (int _rc = (x)) return _rc; } while (0)

namespace qm {
namespace qx {

inline long long waves_of(long long lanes) { return (lanes + 63) / 64; }

#ifdef QM_EMU
typedef int Stream;
typedef int Event;

// Body(args..., wave) for every wavefront; launch2: Body(args..., wave, y), y outermost (a replicate slot or a tile)
template <auto Body, class... A>
int launch(Stream, long long waves, const A&... a) {
  for (long long w = 0; w < waves; ++w) Body(a..., w);
  return 0;
}
template <auto Body, class... A>
int launch2(Stream, long long waves, long long ny, const A&... a) {
  for (long long y = 0; y < ny; ++y) for (long long w = 0; w < waves; ++w) Body(a..., w, y);
  return 0;
}

// out[0 .. n) = exclusive scan of in[0 .. n) (callers pass one element more than they have rows: the last offset is the total)
inline int scan_u32(Stream, DevBuf<unsigned char>&, const u32* in, long long* out, long long n) {
  long long s = 0;
  for (long long i = 0; i < n; ++i) { out[i] = s; s += in[i]; }
  return QM_OK;
}
inline int scan_u64(Stream, DevBuf<unsigned char>&, const u64* in, u64* out, long long n) {
  u64 s = 0;
  for (long long i = 0; i < n; ++i) { out[i] = s; s += in[i]; }
  return QM_OK;
}
// stable sort of n (key, value) pairs by key
inline int sort_pairs(Stream, DevBuf<unsigned char>&, const u32* keyIn, u32* keyOut, const u32* valIn, u32* valOut, long long n) {
  std::vector<long long> perm((size_t)n);
  std::iota(perm.begin(), perm.end(), 0LL);
  std::stable_sort(perm.begin(), perm.end(), [&](long long a, long long b) { return keyIn[a] < keyIn[b]; });
  for (long long i = 0; i < n; ++i) { keyOut[i] = keyIn[perm[(size_t)i]]; valOut[i] = valIn[perm[(size_t)i]]; }
  return QM_OK;
}

inline int fill(Stream, void* p, int byte, size_t bytes) { if (bytes) memset(p, byte, bytes); return QM_OK; }
inline int upload(Stream, void* dst, const void* src, size_t bytes) { if (bytes) memcpy(dst, src, bytes); return QM_OK; }
inline int read(Stream, void* dst, const void* src, size_t bytes) { if (bytes) memcpy(dst, src, bytes); return QM_OK; }
inline int sync(Stream) { return QM_OK; }
inline int tick(Event, Stream) { return QM_OK; }
inline int tock(Event, Event, Stream, int64_t* us) { *us = 0; return QM_OK; }

#else
typedef hipStream_t Stream;
typedef hipEvent_t Event;

#define QX_BLOCK 256           // four wavefronts
// The one kernel of every wave body.  The wavefront's index is wave-uniform by construction: what is decided from it is decided on
// the scalar unit.  A wavefront beyond the last one (the tail of the last block) has nothing to do.
template <auto Body, class... A>
__global__ void __launch_bounds__(QX_BLOCK) wave_kernel(long long waves, A... a) {
  const long long w = uniform(((long long)blockIdx.x * QX_BLOCK + threadIdx.x) >> 6);
  if (w < waves) Body(a..., w);
}
// ... with a second grid dimension: replicate slots, or tiles of replicates (blockIdx.y is uniform as it is)
template <auto Body, class... A>
__global__ void __launch_bounds__(QX_BLOCK) wave2_kernel(long long waves, A... a) {
  const long long w = uniform(((long long)blockIdx.x * QX_BLOCK + threadIdx.x) >> 6);
  if (w < waves) Body(a..., w, (long long)blockIdx.y);
}
inline unsigned wave_blocks(long long waves) { return (unsigned)((waves + QX_BLOCK / 64 - 1) / (QX_BLOCK / 64)); }

template <auto Body, class... A>
hipError_t launch(Stream st, long long waves, A... a) {
  if (waves <= 0) return hipSuccess;
  hipLaunchKernelGGL((wave_kernel<Body, A...>), dim3(wave_blocks(waves)), dim3(QX_BLOCK), 0, st, waves, a...);
  return hipGetLastError();
}
template <auto Body, class... A>
hipError_t launch2(Stream st, long long waves, long long ny, A... a) {
  if (waves <= 0 || ny <= 0) return hipSuccess;
  hipLaunchKernelGGL((wave2_kernel<Body, A...>), dim3(wave_blocks(waves), (unsigned)ny), dim3(QX_BLOCK), 0, st, waves, a...);
  return hipGetLastError();
}

struct U32ToI64 { __device__ __host__ long long operator()(u32 x) const { return (long long)x; } };
// out[0 .. n) = exclusive scan of in[0 .. n) (callers pass one element more than they have rows: the last offset is the total);
// tmp: rocPRIM's scratch, grown as needed
inline int scan_u32(Stream st, DevBuf<unsigned char>& tmp, const u32* in, long long* out, long long n) {
  auto it = rocprim::make_transform_iterator(in, U32ToI64());
  size_t tb = 0; int rc;
  (void)rocprim::exclusive_scan(nullptr, tb, it, out, 0LL, (size_t)n, rocprim::plus<long long>());
  if ((rc = tmp.ensure((int64_t)std::max<size_t>(tb, 1)))) return rc;
  HIPCHK(rocprim::exclusive_scan(tmp.p, tb, it, out, 0LL, (size_t)n, rocprim::plus<long long>(), st));
  return QM_OK;
}
inline int scan_u64(Stream st, DevBuf<unsigned char>& tmp, const u64* in, u64* out, long long n) {
  size_t tb = 0; int rc;
  (void)rocprim::exclusive_scan(nullptr, tb, in, out, (u64)0, (size_t)n, rocprim::plus<u64>());
  if ((rc = tmp.ensure((int64_t)std::max<size_t>(tb, 1)))) return rc;
  HIPCHK(rocprim::exclusive_scan(tmp.p, tb, in, out, (u64)0, (size_t)n, rocprim::plus<u64>(), st));
  return QM_OK;
}
// stable sort of n (key, value) pairs by key
inline int sort_pairs(Stream st, DevBuf<unsigned char>& tmp, const u32* keyIn, u32* keyOut, const u32* valIn, u32* valOut, long long n) {
  size_t tb = 0; int rc;
  (void)rocprim::radix_sort_pairs(nullptr, tb, keyIn, keyOut, valIn, valOut, (size_t)n);
  if ((rc = tmp.ensure((int64_t)std::max<size_t>(tb, 1)))) return rc;
  HIPCHK(rocprim::radix_sort_pairs(tmp.p, tb, keyIn, keyOut, valIn, valOut, (size_t)n, 0, 32, st));
  return QM_OK;
}

inline int fill(Stream st, void* p, int byte, size_t bytes) { HIPCHK(hipMemsetAsync(p, byte, bytes, st)); return QM_OK; }
inline int upload(Stream st, void* dst, const void* src, size_t bytes) { HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st)); return QM_OK; }
// copy to the host and wait for it
inline int read(Stream st, void* dst, const void* src, size_t bytes) {
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return QM_OK;
}
inline int sync(Stream st) { HIPCHK(hipStreamSynchronize(st)); return QM_OK; }
// the timer pair: tick before the work, tock after it (waits for the stream); microseconds, left as they are when the events fail
inline int tick(Event e0, Stream st) { HIPCHK(hipEventRecord(e0, st)); return QM_OK; }
inline int tock(Event e0, Event e1, Stream st, int64_t* us) {
  HIPCHK(hipEventRecord(e1, st));
  HIPCHK(hipEventSynchronize(e1));
  float ms = 0;
  if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) *us = (int64_t)(ms * 1000.0f + 0.5f);
  return QM_OK;
}
#endif

}  // namespace qx
}  // namespace qm
