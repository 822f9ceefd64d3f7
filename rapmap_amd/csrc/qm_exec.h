// qm_exec.h -- what the eight drivers of the estimation objects (qm_eqc_host.inl, qm_quant_host.inl, qm_boot_host.inl, qm_fld_host.inl,
// qm_lib_host.inl, qm_gcb_host.inl, qm_sqb_host.inl, qm_psb_host.inl) run on: a buffer type, the launch of a wave body over a number of wavefronts, two scans and a sort, the host
// operations, and two things every object needs: Base -- device, stream and the two timer events, opened and closed in one place --
// and feed -- host arrays in CSR form cut into parts, uploaded and handed to the caller's function part by part.  Like qm_wave.h it
// has two definitions.  In the library (included by qm_host.hip, after DevBuf, PinBuf, fail and HIPCHK) a launch is a kernel on a
// stream, the scans and the sort are rocPRIM's, and the host operations are HIP's.  With -DQM_EMU (tests/emu only) a buffer is a
// vector, a launch is a loop over the wavefronts, one after the other, and the rest is serial host code: the drivers are the same
// text in both builds, so the CPU suite runs the drivers and not a transcription of them.
// There are two kinds of launch.  launch / launch2: a plain wave body, one wavefront per piece of work.  sweep: a persistent grid of
// `blocks` workgroups whose wavefronts stride over the work themselves (Body gets its index and their number), each with an LDS
// slab of its own when the body wants one; the emulation hands every wavefront a slab filled with 0xA5, so a body must zero what it
// uses.  A kernel that is neither (qm_eqc_host.inl has three) keeps its own kernel and a named launch function with two
// definitions next to its driver.
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

// the persistent grid: Body(args..., wave, 4 * blocks[, slab]) for every wavefront, one after the other, each on SLAB_WORDS words
// refilled with 0xA5A5A5A5
template <auto Body, int SLAB_WORDS = 0, class... A>
int sweep(Stream, int blocks, const A&... a) {
  const long long nWaves = 4LL * blocks;
  std::vector<u32> slab((size_t)SLAB_WORDS);
  for (long long w = 0; w < nWaves; ++w) {
    if constexpr (SLAB_WORDS > 0) { slab.assign((size_t)SLAB_WORDS, 0xA5A5A5A5u); Body(a..., w, nWaves, slab.data()); }
    else Body(a..., w, nWaves);
  }
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
inline void elapsed(Event, Event, int64_t* us) { *us = 0; }
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

// The one kernel of every persistent grid: every wavefront of the `blocks` workgroups runs Body(args..., wave, waves in the grid
// [, slab]), slab: SLAB_WORDS words of LDS of its own.  blocks <= 0 launches nothing.
template <auto Body, int SLAB_WORDS, class... A>
__global__ void __launch_bounds__(QX_BLOCK) sweep_kernel(A... a) {
  const long long w = uniform(((long long)blockIdx.x * QX_BLOCK + threadIdx.x) >> 6), nWaves = (long long)gridDim.x * (QX_BLOCK / 64);
  if constexpr (SLAB_WORDS > 0) {
    __shared__ alignas(8) u32 slab[QX_BLOCK / 64][SLAB_WORDS];     // (a body may keep 64-bit words in an even SLAB_WORDS)
    Body(a..., w, nWaves, (QM_LDS(u32)*)&slab[threadIdx.x >> 6][0]);
  }
  else Body(a..., w, nWaves);
}
template <auto Body, int SLAB_WORDS = 0, class... A>
hipError_t sweep(Stream st, int blocks, A... a) {
  if (blocks <= 0) return hipSuccess;
  hipLaunchKernelGGL((sweep_kernel<Body, SLAB_WORDS, A...>), dim3((unsigned)blocks), dim3(QX_BLOCK), 0, st, a...);
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
// the timer pair: tick before the work, tock after it (waits for the stream); microseconds, left as they are when the events fail.
// A driver that waits for a read-back anyway ticks both events itself and asks for `elapsed` after the read: no second wait.
inline int tick(Event e, Stream st) { HIPCHK(hipEventRecord(e, st)); return QM_OK; }
inline void elapsed(Event e0, Event e1, int64_t* us) {
  float ms = 0;
  if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) *us = (int64_t)(ms * 1000.0f + 0.5f);
}
inline int tock(Event e0, Event e1, Stream st, int64_t* us) {
  HIPCHK(hipEventRecord(e1, st));
  HIPCHK(hipEventSynchronize(e1));
  elapsed(e0, e1, us);
  return QM_OK;
}
#endif

// What every estimation object owns: its device, a stream and the two events of its timer.  open: `who` names the object's create
// function in the messages; with `borrowed` the stream is another object's (a qm_boot runs on its quant's) and only the events are
// made.  close gives back what open made -- a borrowed stream is waited for and left alone.  The emulation has nothing to make.
struct Base {
  int device = 0, numCU = 256;
  Stream stream{}; Event ev0{}, ev1{};
  bool ownsStream = true;
  int open(const char* who, int dev, int cus, const Stream* borrowed = nullptr) {
    device = dev; numCU = cus; ownsStream = !borrowed;
    if (borrowed) stream = *borrowed;
#ifndef QM_EMU
    if (ownsStream && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) return fail(QM_E_NOGPU, "%s: stream", who);
    if (hipEventCreate(&ev0) != hipSuccess || hipEventCreate(&ev1) != hipSuccess) return fail(QM_E_NOGPU, "%s: events", who);
#endif
    return QM_OK;
  }
  void close() {
#ifndef QM_EMU
    hipSetDevice(device);
    if (stream) hipStreamSynchronize(stream);
    if (ev0) hipEventDestroy(ev0);
    if (ev1) hipEventDestroy(ev1);
    if (stream && ownsStream) hipStreamDestroy(stream);
#endif
  }
};

// Host arrays in parts.  The n units' items lie in `items` (itemBytes each) from offsets[u] to offsets[u + 1]; perUnit (optional)
// has one word per unit.  A part always takes one unit and is extended while it has fewer than maxUnits units and the next unit
// still fits into maxItems items.  Per part the offsets are rebased to 0 and go up with the part's items and words into the
// buffers of `in`; the stream is waited for (the host vector is reused), and part(off, items, perUnit, u0, nu, nItems) gets the
// device pointers -- items null for a part without items, perUnit null when there is none.  who / unit / item: for the messages.
struct FeedBuf { DevBuf<long long> off; DevBuf<unsigned char> items; DevBuf<u64> perUnit; std::vector<long long> h_off; };
template <class Part>
int feed(Stream st, FeedBuf& in, const char* who, const char* unit, const char* item, int64_t n, const int64_t* offsets, const void* items, size_t itemBytes,
         const uint64_t* perUnit, int64_t maxUnits, int64_t maxItems, Part&& part) {
  if (n < 0 || (n > 0 && !offsets)) return fail(QM_E_ARG, "%s: bad argument", who);
  for (int64_t i = 0; i < n; ++i) if (offsets[i + 1] < offsets[i]) return fail(QM_E_ARG, "%s: offsets decrease at %s %lld", who, unit, (long long)i);
  if (n > 0 && offsets[n] > offsets[0] && !items) return fail(QM_E_ARG, "%s: null %s", who, item);
  int rc;
  for (int64_t u0 = 0; u0 < n;) {
    int64_t u1 = u0 + 1;
    while (u1 < n && u1 - u0 < maxUnits && offsets[u1 + 1] - offsets[u0] <= maxItems) ++u1;
    const int64_t nu = u1 - u0, ni = offsets[u1] - offsets[u0];
    in.h_off.resize((size_t)nu + 1);
    for (int64_t i = 0; i <= nu; ++i) in.h_off[(size_t)i] = offsets[u0 + i] - offsets[u0];
    if ((rc = in.off.ensure(nu + 1)) || (ni > 0 && (rc = in.items.ensure(ni * (int64_t)itemBytes))) || (perUnit && (rc = in.perUnit.ensure(nu)))) return rc;
    QXCHK(upload(st, in.off, in.h_off.data(), (size_t)(nu + 1) * 8));
    if (ni > 0) QXCHK(upload(st, in.items, (const unsigned char*)items + (size_t)offsets[u0] * itemBytes, (size_t)ni * itemBytes));
    if (perUnit) QXCHK(upload(st, in.perUnit, perUnit + u0, (size_t)nu * 8));
    QXCHK(sync(st));
    if ((rc = part((const long long*)in.off.p, ni > 0 ? (const unsigned char*)in.items.p : nullptr, perUnit ? (const u64*)in.perUnit.p : nullptr, u0, nu, ni))) return rc;
    u0 = u1;
  }
  return QM_OK;
}

}  // namespace qx
}  // namespace qm
