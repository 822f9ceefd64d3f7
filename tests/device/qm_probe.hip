// tests/device/qm_probe.hip -- TEST-ONLY device probes (libqm_probe.so; nothing of it is linked into libqmap_mi355.so).  Each entry point
// runs one wave body of the product's source by itself on the GPU, on inputs the caller chooses, so that the device edition of the body can
// be held to its lane emulation (tests/emu) unit by unit:
//   qp_wave       the primitives of qm_wave.h, key_count and the pieces of qm_sweep.h (qm_wave_probe.inl, the body tests/emu/qm_emu_wave.cpp compiles with -DQM_EMU)
//   qp_h2m        lean_h2m, lean_h2m_loop, lean_h2m_tiles<false / true> of qm_lean.inl on a stash in LDS          (tests/emu/qm_emu_h2m.cpp)
//   qp_ksw_rows   sel_ksw_extz2_rows<RING> of qm_sel.inl, four alignments per wavefront                           (tests/emu/qm_emu.cpp)
//   qp_ksw_rows8  sel_ksw_extz2_rows_reg<.., true, 2>, eight alignments of one shape per wavefront
//   qp_sel_side   sel_side_score<G> with SelRed2 / 4 / 8 / 16, 256 / G questions per block as qm_sel_score_kernel launches it    (tests/emu/qm_emu_sel.cpp)
//   qp_sel_strip  sel_tasks_strip, four alignments per wavefront as qm_sel_strip_kernel launches it
// An entry point is self-contained: host arrays in, hipSetDevice(0), allocate, copy, ONE launch, synchronise, copy back, free; it returns the
// hipError_t (hipErrorInvalidValue for an argument outside what the body is written for -- checked here, before anything is launched).
// One wave of the caller's = one wavefront; blocks of four wavefronts (the ksw2 kernels: as many as the product's launch wrapper gives that
// ring), at least two blocks; all 64 lanes of a wavefront are active.
#include "../../rapmap_amd/csrc/qm_lean.inl"
#include "qm_wave_probe.inl"

#include <string.h>
#include <type_traits>
#include <vector>

using namespace qm;

namespace {

// device buffers of one entry point: freed together, the first error kept
struct ProbeBufs {
  std::vector<void*> p;
  hipError_t err = hipSuccess;
  template <typename T> T* put(const T* host, size_t n) {                  // allocate n elements (at least one) and copy the host's in
    void* d = nullptr;
    if (err == hipSuccess) err = hipMalloc(&d, (n ? n : 1) * sizeof(T));
    if (err == hipSuccess) p.push_back(d); else return nullptr;
    if (host && n) err = hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice);
    return (T*)d;
  }
  template <typename T> T* fill(size_t n, int byte) {                      // allocate n elements set to one byte value
    T* d = put<T>(nullptr, n);
    if (err == hipSuccess) err = hipMemset(d, byte, (n ? n : 1) * sizeof(T));
    return d;
  }
  template <typename T> void get(T* host, const T* dev, size_t n) { if (err == hipSuccess && n) err = hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost); }
  void sync() { if (err == hipSuccess) err = hipGetLastError(); if (err == hipSuccess) err = hipDeviceSynchronize(); }
  ~ProbeBufs() { for (void* d : p) (void)hipFree(d); }
};

unsigned blocks_for(int nwaves, int wavesPerBlock) { const int b = (nwaves + wavesPerBlock - 1) / wavesPerBlock; return (unsigned)(b < 2 ? 2 : b); }

// ---------------------------------------------------------------------------------------------------------------- the primitives
__global__ __launch_bounds__(256) void qp_wave_kernel(int op, int nw, const int* prm, const u64* a, const u64* b, const u64* c, const u64* d,
                                                      const unsigned char* mem, u64* atom, u64* out) {
  __shared__ u32 lds[4][QP_LDSB / 4];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wave = (int)blockIdx.x * 4 + wv;
  if (wave >= nw) return;                                                  // (a whole wavefront leaves: the others keep all their lanes)
  const size_t o = (size_t)wave * 64;
  (void)probe_wave(op, __builtin_amdgcn_readfirstlane(prm[wave]), a + o, b + o, c + o, d + o, mem + (size_t)wave * QP_MEMB, atom + wave, lds[wv],
                   out + o * QP_NOUT);
}

// ---------------------------------------------------------------------------------------------------------------- lean_h2m
// hdr: per wave {n, m, minIdx, isRC}; stash: per wave 64 x {tid, pos, qp, iv}, all 64 slots as the caller wants the LDS to hold them
__global__ __launch_bounds__(256) void qp_h2m_kernel(int which, int nw, const int* hdr, const u32* stash, int* cnt, u64* elem, unsigned char* keep, int* slot) {
  __shared__ LeanSuf sufs[4][QM_LEAN_SUF];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wave = (int)blockIdx.x * 4 + wv;
  if (wave >= nw) return;
  const int lane = (int)(threadIdx.x & 63);
  QM_LDS(LeanSuf)* suf = (QM_LDS(LeanSuf)*)sufs[wv];
  const u32* st = stash + ((size_t)wave * 64 + lane) * 4;
  suf[lane].tid = st[0]; suf[lane].pos = st[1]; suf[lane].qp = st[2]; suf[lane].iv = st[3];
  wave_fence();
  LeanStrand S;
  S.sufN = uniform(hdr[4 * wave]); S.n = uniform(hdr[4 * wave + 1]); S.minIdx = uniform(hdr[4 * wave + 2]); S.minSpan = 0; S.cov = 0;
  const bool isRC = uniform(hdr[4 * wave + 3]) != 0;
  LV<u64> e; LV<bool> k; LV<int> s;
  e.v[0] = 0x5A5A5A5A5A5A5A5AULL; k.v[0] = true; s.v[0] = -77;             // (nothing of the caller's survives the pass)
  int c = -1;
  if (which == 0) c = lean_h2m(suf, S, isRC, e, k, s);
  else if (which == 1) c = lean_h2m_loop(suf, S, isRC, e, k, s);
  else if (which == 2) c = lean_h2m_tiles<false>(suf, S, isRC, e, k, s);
  else if (which == 3) c = lean_h2m_tiles<true>(suf, S, isRC, e, k, s);
  const size_t o = (size_t)wave * 64 + lane;
  elem[o] = e.v[0]; keep[o] = k.v[0] ? 1 : 0; slot[o] = s.v[0];
  if (lane == 0) cnt[wave] = c;
}

// ---------------------------------------------------------------------------------------------------------------- the ksw2 row kernels
struct KswArgs { int a, b, q, e, w; };
// One alignment's block as tests/emu/qm_emu.cpp (ksw_rows_run) leaves it: 0xAB everywhere, then only what sel_tasks_stage writes for an alignment
// of this size -- the images up to tlen16 + qlen + 48.  The 64 lanes of the wavefront stride over the bytes.
template <typename Row, int MAXLEN>
__device__ void qp_stage(Row* B, int lane, bool real, int qlen, int tlen, const unsigned char* query, const unsigned char* target) {
  unsigned char* raw = (unsigned char*)B;
  for (int i = lane; i < (int)sizeof(Row); i += 64) raw[i] = 0xAB;
  wave_fence();
  if (!real) return;
  const int tlen16 = (tlen + 15) / 16 * 16;
  for (int i = lane; i < MAXLEN + 40 && i < tlen16 + qlen + 48; i += 64) {
    B->QX[i] = (i >= 16 && i < 16 + qlen) ? query[i - 16] : (unsigned char)0;
    const int j = i - tlen16;
    B->TX[i] = i < tlen ? target[i] : (i < tlen16 ? (unsigned char)0 : (j < qlen ? query[qlen - 1 - j] : (unsigned char)0));
  }
}
__device__ void qp_matrix(const KswArgs& K, signed char* mat) {            // (sel_ksw_matrix)
  int a = K.a < 0 ? -K.a : K.a, b = K.b > 0 ? -K.b : K.b;
  for (int i = 0; i < 4; ++i) { for (int j = 0; j < 4; ++j) mat[i * 5 + j] = (signed char)(i == j ? a : b); mat[i * 5 + 4] = 0; }
  for (int j = 0; j < 5; ++j) mat[20 + j] = 0;
}
// hdr: per wave 4 x {qlen, tlen, query offset, target offset} (offsets into seq; an idle row: 0, 0); out: 4 scores per wave.
// rows: the wave's four blocks.
template <int RING, int MAXLEN>
__device__ void qp_ksw_rows_wave(int wave, const int* hdr, const unsigned char* seq, const KswArgs& K, KswRowT<RING, MAXLEN>* rows, int* out) {
  const int lane = (int)(threadIdx.x & 63);
  for (int g = 0; g < 4; ++g) {
    const int* h = hdr + ((size_t)wave * 4 + g) * 4;
    const int ql = uniform(h[0]), tl = uniform(h[1]);
    qp_stage<KswRowT<RING, MAXLEN>, MAXLEN>(rows + g, lane, true, ql, tl, seq + uniform(h[2]), seq + uniform(h[3]));
  }
  wave_fence();
  const int* h = hdr + ((size_t)wave * 4 + (lane >> 4)) * 4;
  LV<int> ql, tl, sc;
  ql.v[0] = h[0]; tl.v[0] = h[1];
  signed char mat[25];
  qp_matrix(K, mat);
  sel_ksw_extz2_rows<RING, MAXLEN>(ql, tl, rows, mat, K.q, K.e, K.w, sc);
  if ((lane & 15) == 0) out[(size_t)wave * 4 + (lane >> 4)] = sc.v[0];
}
// the blocks in LDS, four per wavefront (qm_sel_align_kernel: 64 slots: four wavefronts per block, 128: four, 1024: two)
template <int RING, int WAVES>
__global__ __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(8, 8))) void qp_ksw_rows_kernel(int nw, const int* hdr, const unsigned char* seq, KswArgs K, int* out) {
  __shared__ KswRowT<RING, QM_KSW_MAXLEN> rows[WAVES][4];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wave = (int)blockIdx.x * WAVES + wv;
  if (wave >= nw) return;
  qp_ksw_rows_wave<RING, QM_KSW_MAXLEN>(wave, hdr, seq, K, rows[wv], out);
}
// the register edition's blocks, eight per wavefront (qm_sel_align2_kernel): four alignments use the first four
__global__ __launch_bounds__(256) void qp_ksw_rows32_kernel(int nw, const int* hdr, const unsigned char* seq, KswArgs K, int* out) {
  __shared__ KswRowT<32, QM_KSW_MAXLEN> rows[4][8];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wave = (int)blockIdx.x * 4 + wv;
  if (wave >= nw) return;
  qp_ksw_rows_wave<32, QM_KSW_MAXLEN>(wave, hdr, seq, K, rows[wv], out);
}
// the 4096-slot ring: the blocks in device memory, four per wavefront, two wavefronts per block (qm_sel_align_gmem_kernel)
__global__ __launch_bounds__(128) void qp_ksw_rows_gmem_kernel(int nw, const int* hdr, const unsigned char* seq, KswArgs K,
                                                               KswRowT<QM_KSW_RING_GMEM, QM_KSW_MAXLEN_LONG>* rows, int* out) {
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wave = (int)blockIdx.x * 2 + wv;
  if (wave >= nw) return;
  qp_ksw_rows_wave<QM_KSW_RING_GMEM, QM_KSW_MAXLEN_LONG>(wave, hdr, seq, K, rows + (size_t)wave * 4, out);
}
// hdr: per wave {n, qlen, tlen, 0} and 8 x {query offset, target offset}: 20 ints; out: 8 scores per wave
__global__ __launch_bounds__(256) void qp_ksw_rows8_kernel(int nw, const int* hdr, const unsigned char* seq, KswArgs K, int* out) {
  __shared__ KswRowT<32, QM_KSW_MAXLEN> rows[4][8];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wave = (int)blockIdx.x * 4 + wv;
  if (wave >= nw) return;
  const int lane = (int)(threadIdx.x & 63);
  const int* h = hdr + (size_t)wave * 20;
  const int n = uniform(h[0]), qlen = uniform(h[1]), tlen = uniform(h[2]);
  for (int g = 0; g < 8; ++g)
    qp_stage<KswRowT<32, QM_KSW_MAXLEN>, QM_KSW_MAXLEN>(&rows[wv][g], lane, g < n, qlen, tlen, seq + uniform(h[4 + 2 * g]), seq + uniform(h[5 + 2 * g]));
  wave_fence();
  LV<int> ql[2], tl[2], sc[2];
  for (int s = 0; s < 2; ++s) { const int g = 4 * s + (lane >> 4); ql[s].v[0] = g < n ? qlen : 0; tl[s].v[0] = g < n ? tlen : 0; }
  signed char mat[25];
  qp_matrix(K, mat);
  sel_ksw_extz2_rows_reg<QM_KSW_MAXLEN, true, 2>(ql, tl, qlen, tlen, rows[wv], mat, K.q, K.e, K.w, sc);
  if ((lane & 15) == 0) for (int s = 0; s < 2; ++s) out[(size_t)wave * 8 + 4 * s + (lane >> 4)] = sc[s].v[0];
}

// ---------------------------------------------------------------------------------------------------------------- the -s question scorer, the strip alignments
// qm_sel_score_kernel<G> and qm_sel_strip_kernel of qm_kernels.hip, word for word: 256-thread blocks, 256 / G questions per block and trip with the
// product's own group reductions (SelRed2 / 4 / 8 / 16, qm_sel.inl); four strip tasks per wavefront on __shared__ StripMem[4]
template <int G>
__global__ __launch_bounds__(256) void qp_sel_side_kernel(PairBatch P, SelBatch A) {
  const unsigned long long n = *A.nsides;
  constexpr int PER = 256 / G;
  const int l = (int)(threadIdx.x & (G - 1));
  typename std::conditional<G == 16, SelRed16, typename std::conditional<G == 8, SelRed8, typename std::conditional<G == 4, SelRed4, SelRed2>::type>::type>::type red;
  for (unsigned long long x = (unsigned long long)blockIdx.x * PER + (threadIdx.x / G); x < n; x += (unsigned long long)gridDim.x * PER)
    sel_side_score<G>(P, A, (long long)x, l, red);
}
__global__ __launch_bounds__(256) void qp_sel_strip_kernel(SelBatch A) {
  __shared__ StripMem mem[4];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const unsigned long long nt = *A.ntasks2;
  for (unsigned long long t = ((unsigned long long)blockIdx.x * 4 + wave) * 4; t < nt; t += (unsigned long long)gridDim.x * 16) sel_tasks_strip(A, t, nt, mem[wave]);
}
// blocks for n items, `per` of them per block and trip: at least two, and about half as many as one trip would take (the stride loop runs)
unsigned blocks_two_trips(long long n, int per) { const long long b = ((n + per - 1) / per + 1) / 2; return (unsigned)(b < 2 ? 2 : b); }

// a sequence [off, off + len) must lie inside the nseq bytes the caller passed
bool seq_ok(long long off, long long len, long long nseq) { return off >= 0 && len >= 0 && off + len <= nseq; }

}  // namespace

extern "C" {

const char* qp_error_string(int err) { return hipGetErrorString((hipError_t)err); }
int qp_n_ops(void) { return QP_NOPS; }
const char* qp_op_name(int op) {
#define QP_NAME(n) #n,
  static const char* const names[] = {QP_OPS(QP_NAME)};
#undef QP_NAME
  return op >= 0 && op < QP_NOPS ? names[op] : nullptr;
}
int qp_memb(void) { return QP_MEMB; }
int qp_nout(void) { return QP_NOUT; }
int qp_h2m_tile_lo(void) { return QM_H2M_TILE_LO; }
int qp_h2m_tile_hi(void) { return QM_H2M_TILE_HI; }
int qp_ksw_ring_slots(int w) { return sel_ksw_ring_slots(w); }

// nw waves of op: prm[nw], a / b / c / d [nw * 64], mem[nw * QP_MEMB], atom[nw] (in: the words' start values, out: what the wave left),
// out[nw * QP_NOUT * 64] (filled with the byte 0xEE before the launch)
int qp_wave(int op, int nw, const int* prm, const u64* a, const u64* b, const u64* c, const u64* d, const unsigned char* mem, u64* atom, u64* out) {
  if (op < 0 || op >= QP_NOPS || nw < 1) return (int)hipErrorInvalidValue;
  for (int w = 0; w < nw; ++w) {
    if (op == QP_group_min && !(prm[w] == 1 || prm[w] == 2 || prm[w] == 4 || prm[w] == 8 || prm[w] == 16 || prm[w] == 32 || prm[w] == 64)) return (int)hipErrorInvalidValue;
    if (op == QP_group_sum_f64 && prm[w] != 8 && prm[w] != 16) return (int)hipErrorInvalidValue;
    if (op == QP_unit_bounds && !QP_UNIT_BOUNDS_OK(prm[w], a[(size_t)w * 64], b[(size_t)w * 64])) return (int)hipErrorInvalidValue;
    if (op == QP_slab_flush && (prm[w] < 1 || prm[w] > QP_LDSB / 4)) return (int)hipErrorInvalidValue;
  }
  hipError_t e = hipSetDevice(0);
  if (e != hipSuccess) return (int)e;
  ProbeBufs B;
  const size_t n = (size_t)nw * 64;
  const int* dprm = B.put(prm, nw);
  const u64 *da = B.put(a, n), *db = B.put(b, n), *dc = B.put(c, n), *dd = B.put(d, n);
  const unsigned char* dmem = B.put(mem, (size_t)nw * QP_MEMB);
  u64* datom = B.put(atom, nw);
  u64* dout = B.fill<u64>(n * QP_NOUT, 0xEE);
  if (B.err != hipSuccess) return (int)B.err;
  hipLaunchKernelGGL(qp_wave_kernel, dim3(blocks_for(nw, 4)), dim3(256), 0, 0, op, nw, dprm, da, db, dc, dd, dmem, datom, dout);
  B.sync();
  B.get(atom, datom, nw);
  B.get(out, dout, n * QP_NOUT);
  return (int)B.err;
}

// which: 0 lean_h2m, 1 lean_h2m_loop, 2 lean_h2m_tiles<false> (n <= 32), 3 lean_h2m_tiles<true> (n <= 8).  hdr: nw x {n, m, minIdx, isRC}; stash: nw x 64 x
// {tid, pos, qp, iv} (the slots from n on: whatever the LDS is to hold there).  Out: cnt[nw], elem / keep / slot [nw * 64].
int qp_h2m(int which, int nw, const int* hdr, const u32* stash, int* cnt, u64* elem, unsigned char* keep, int* slot) {
  if (which < 0 || which > 3 || nw < 1) return (int)hipErrorInvalidValue;
  for (int w = 0; w < nw; ++w) {
    const int n = hdr[4 * w], m = hdr[4 * w + 1], mi = hdr[4 * w + 2];
    if (n < 0 || n > QM_LEAN_SUF || m < 1 || m > QM_LEAN_MAXIV || mi < 0 || mi >= m) return (int)hipErrorInvalidValue;
    if ((which == 2 && n > 32) || (which == 3 && n > 8)) return (int)hipErrorInvalidValue;
  }
  hipError_t e = hipSetDevice(0);
  if (e != hipSuccess) return (int)e;
  ProbeBufs B;
  const size_t n = (size_t)nw * 64;
  const int* dhdr = B.put(hdr, (size_t)nw * 4);
  const u32* dst = B.put(stash, n * 4);
  int* dcnt = B.fill<int>(nw, 0xEE); u64* delem = B.fill<u64>(n, 0xEE); unsigned char* dkeep = B.fill<unsigned char>(n, 0xEE); int* dslot = B.fill<int>(n, 0xEE);
  if (B.err != hipSuccess) return (int)B.err;
  hipLaunchKernelGGL(qp_h2m_kernel, dim3(blocks_for(nw, 4)), dim3(256), 0, 0, which, nw, dhdr, dst, dcnt, delem, dkeep, dslot);
  B.sync();
  B.get(cnt, dcnt, nw); B.get(elem, delem, n); B.get(keep, dkeep, n); B.get(slot, dslot, n);
  return (int)B.err;
}

// nw wavefronts of four alignments: hdr[nw * 16] = 4 x {qlen, tlen, query offset, target offset} into seq[nseq] (nt4 codes); an idle row: qlen = tlen = 0.
// ring: 32 / 64 / 128 / 1024 slots in LDS, 4096 in device memory; it must hold the band (sel_ksw_ring_slots(w) <= ring).  out[nw * 4].
int qp_ksw_rows(int ring, int nw, const int* hdr, const unsigned char* seq, long long nseq, int a, int b, int q, int e_, int w, int* out) {
  if (nw < 1 || !(ring == 32 || ring == 64 || ring == 128 || ring == 1024 || ring == QM_KSW_RING_GMEM) || sel_ksw_ring_slots(w) > ring) return (int)hipErrorInvalidValue;
  const int maxq = ring == QM_KSW_RING_GMEM ? QM_MAX_LONG_READ_LEN : QM_MAX_READ_LEN, maxt = ring == QM_KSW_RING_GMEM ? QM_KSW_MAXLEN_LONG : QM_KSW_MAXLEN;
  for (int i = 0; i < nw * 4; ++i) {
    const int* h = hdr + 4 * i;
    if (h[0] < 0 || h[0] > maxq || h[1] < 0 || h[1] > maxt || !seq_ok(h[2], h[0], nseq) || !seq_ok(h[3], h[1], nseq)) return (int)hipErrorInvalidValue;
  }
  hipError_t e = hipSetDevice(0);
  if (e != hipSuccess) return (int)e;
  ProbeBufs B;
  const int* dhdr = B.put(hdr, (size_t)nw * 16);
  const unsigned char* dseq = B.put(seq, (size_t)nseq);
  int* dout = B.fill<int>((size_t)nw * 4, 0xEE);
  typedef KswRowT<QM_KSW_RING_GMEM, QM_KSW_MAXLEN_LONG> GRow;
  GRow* drows = ring == QM_KSW_RING_GMEM ? B.put<GRow>(nullptr, (size_t)nw * 4) : nullptr;
  if (B.err != hipSuccess) return (int)B.err;
  const KswArgs K = {a, b, q, e_, w};
  switch (ring) {
    case 32: hipLaunchKernelGGL(qp_ksw_rows32_kernel, dim3(blocks_for(nw, 4)), dim3(256), 0, 0, nw, dhdr, dseq, K, dout); break;
    case 64: hipLaunchKernelGGL((qp_ksw_rows_kernel<64, 4>), dim3(blocks_for(nw, 4)), dim3(256), 0, 0, nw, dhdr, dseq, K, dout); break;
    case 128: hipLaunchKernelGGL((qp_ksw_rows_kernel<128, 4>), dim3(blocks_for(nw, 4)), dim3(256), 0, 0, nw, dhdr, dseq, K, dout); break;
    case 1024: hipLaunchKernelGGL((qp_ksw_rows_kernel<1024, 2>), dim3(blocks_for(nw, 2)), dim3(128), 0, 0, nw, dhdr, dseq, K, dout); break;
    default: hipLaunchKernelGGL(qp_ksw_rows_gmem_kernel, dim3(blocks_for(nw, 2)), dim3(128), 0, 0, nw, dhdr, dseq, K, drows, dout); break;
  }
  B.sync();
  B.get(out, dout, (size_t)nw * 4);
  return (int)B.err;
}

// nw wavefronts of eight alignments of one shape, n of them real: hdr[nw * 20] = {n, qlen, tlen, 0} and 8 x {query offset, target offset}.  Bands 0 .. 15.
int qp_ksw_rows8(int nw, const int* hdr, const unsigned char* seq, long long nseq, int a, int b, int q, int e_, int w, int* out) {
  if (nw < 1 || w < 0 || w > 15) return (int)hipErrorInvalidValue;
  for (int i = 0; i < nw; ++i) {
    const int* h = hdr + 20 * i;
    if (h[0] < 1 || h[0] > 8 || h[1] < 1 || h[1] > QM_MAX_READ_LEN || h[2] < 1 || h[2] > QM_KSW_MAXLEN) return (int)hipErrorInvalidValue;
    for (int g = 0; g < 8; ++g)
      if (g < h[0] ? (!seq_ok(h[4 + 2 * g], h[1], nseq) || !seq_ok(h[5 + 2 * g], h[2], nseq)) : (h[4 + 2 * g] != 0 || h[5 + 2 * g] != 0)) return (int)hipErrorInvalidValue;
  }
  hipError_t e = hipSetDevice(0);
  if (e != hipSuccess) return (int)e;
  ProbeBufs B;
  const int* dhdr = B.put(hdr, (size_t)nw * 20);
  const unsigned char* dseq = B.put(seq, (size_t)nseq);
  int* dout = B.fill<int>((size_t)nw * 8, 0xEE);
  if (B.err != hipSuccess) return (int)B.err;
  const KswArgs K = {a, b, q, e_, w};
  hipLaunchKernelGGL(qp_ksw_rows8_kernel, dim3(blocks_for(nw, 4)), dim3(256), 0, 0, nw, dhdr, dseq, K, dout);
  B.sync();
  B.get(out, dout, (size_t)nw * 8);
  return (int)B.err;
}

int qp_sel_max_read_len(void) { return QM_MAX_READ_LEN; }

// nq questions in ONE launch of qp_sel_side_kernel<G> (G: 2, 4, 8 or 16 lanes per question), one unit and one hit per question -- the arguments and
// the answers of tests/emu/qm_emu_sel.cpp's qe_sel_side (its strip pass is qp_sel_strip here).  reads[roffs[nq]]: question x asks about
// reads[roffs[x] .. roffs[x + 1]); text[ntext] with ntx transcripts txp_off / txp_len; qd: nq x {tid, pos, fwd, chain status, multi-mapping unit};
// prm: {policy, match, mismatch, gap open, gap extend, band}.  Out, per question: kind, tsc (0x5A5A5A5A: never written), key, task[9] = {written,
// read offset, target offset, gslot, rl, roff, rlen, tlen1, fwd} (written 0: tasks[x] still holds the 0xEE it was filled with; the rest is 0 then).
int qp_sel_side(int G, int nq, const unsigned char* reads, const long long* roffs, const unsigned char* text, long long ntext, int ntx, const u32* txp_off,
                const int* txp_len, const int* qd, const int* prm, int* kind, int* tsc, u64* key, long long* task) {
  if (!(G == 2 || G == 4 || G == 8 || G == 16) || nq < 1 || ntx < 1 || roffs[0] < 0) return (int)hipErrorInvalidValue;
  for (int t = 0; t < ntx; ++t) if (txp_len[t] < 0 || (long long)txp_off[t] + txp_len[t] > ntext) return (int)hipErrorInvalidValue;
  for (int x = 0; x < nq; ++x) {
    const int* d = qd + 5 * x;
    if (roffs[x + 1] < roffs[x] || roffs[x + 1] - roffs[x] > QM_MAX_LONG_READ_LEN || d[0] < 0 || d[0] >= ntx || d[1] < -(1 << 24) || d[1] > (1 << 24)) return (int)hipErrorInvalidValue;
  }
  hipError_t e = hipSetDevice(0);
  if (e != hipSuccess) return (int)e;
  const size_t n = (size_t)nq;
  std::vector<u32> cnt(n + 1, 0);
  std::vector<qm_hit> tmp(n);
  std::vector<SelSide> sides(n);
  memset(sides.data(), 0xEE, sizeof(SelSide) * n);
  for (size_t x = 0; x < n; ++x) {
    const int* d = qd + 5 * x;
    qm_hit h; memset(&h, 0, sizeof(h));
    h.tid = (u32)d[0]; h.pos = d[1]; h.fwd = d[2] ? 1 : 0; h.mate_is_fwd = 1; h.read_len = (u32)(roffs[x + 1] - roffs[x]); h.aln_score = d[3];
    tmp[x] = h;
    cnt[x] = d[4] ? 2u : 1u;
    sides[x].u = (long long)x; sides[x].g = 2 * (long long)x; sides[x].nth = 0;
  }
  // (the sequences with sixteen bytes of 0xA5 behind them: the word loads stay inside [0, len), and if one did not it would stay inside the allocation)
  std::vector<unsigned char> hr(reads, reads + roffs[nq]), ht(text, text + ntext);
  hr.resize(hr.size() + 16, 0xA5); ht.resize(ht.size() + 16, 0xA5);
  const u64 nsides = (u64)n;
  ProbeBufs B;
  const unsigned char* dreads = B.put(hr.data(), hr.size()); const unsigned char* dtext = B.put(ht.data(), ht.size());
  const long long* droffs = B.put(roffs, n + 1);
  const u32* dtoff = B.put(txp_off, (size_t)ntx); const int* dtlen = B.put(txp_len, (size_t)ntx);
  u32* dcnt = B.put(cnt.data(), n + 1); qm_hit* dtmp = B.put(tmp.data(), n); SelSide* dsides = B.put(sides.data(), n);
  u64* dnsides = B.put(&nsides, 1);
  SelTask* dtasks = B.fill<SelTask>(n, 0xEE);
  int* dtsc = B.fill<int>(2 * n, 0x5A); int* dtref = B.fill<int>(2 * n, 0x5A);
  u64* dtorder2 = B.fill<u64>(n, 0); u64* dntasks2 = B.fill<u64>(1, 0);
  if (B.err != hipSuccess) return (int)B.err;
  PairBatch P; memset(&P, 0, sizeof(P));
  P.n = nq; P.paired = 0; P.off1 = droffs; P.off2 = droffs; P.cnt = dcnt; P.max_num_hits = 200;
  SelBatch A; memset(&A, 0, sizeof(A));
  A.seq1 = dreads; A.seq2 = dreads; A.text = dtext; A.txp_off = dtoff; A.txp_len = dtlen; A.tmp = dtmp;
  A.tsc = dtsc; A.tref = dtref; A.sides = dsides; A.nsides = dnsides; A.tasks = dtasks; A.torder2 = dtorder2; A.ntasks2 = dntasks2; A.u0 = 0; A.u1 = nq;
  A.policy = prm[0]; A.match = prm[1]; A.mismatch = prm[2]; A.gap_open = prm[3]; A.gap_extend = prm[4]; A.bandwidth = prm[5];
  A.min_score_fraction = 0.65;
  const unsigned nb = blocks_two_trips(nq, 256 / G);
  switch (G) {
    case 2: hipLaunchKernelGGL(qp_sel_side_kernel<2>, dim3(nb), dim3(256), 0, 0, P, A); break;
    case 4: hipLaunchKernelGGL(qp_sel_side_kernel<4>, dim3(nb), dim3(256), 0, 0, P, A); break;
    case 8: hipLaunchKernelGGL(qp_sel_side_kernel<8>, dim3(nb), dim3(256), 0, 0, P, A); break;
    default: hipLaunchKernelGGL(qp_sel_side_kernel<16>, dim3(nb), dim3(256), 0, 0, P, A); break;
  }
  B.sync();
  std::vector<SelTask> tasks(n); std::vector<int> tscv(2 * n);
  B.get(sides.data(), dsides, n); B.get(tasks.data(), dtasks, n); B.get(tscv.data(), dtsc, 2 * n);
  if (B.err != hipSuccess) return (int)B.err;
  std::vector<unsigned char> fill(sizeof(SelTask), 0xEE);
  for (size_t x = 0; x < n; ++x) {
    kind[x] = sides[x].kind; key[x] = sides[x].key; tsc[x] = tscv[2 * x];
    long long* o = task + 9 * x;
    for (int i = 0; i < 9; ++i) o[i] = 0;
    if (memcmp(&tasks[x], fill.data(), sizeof(SelTask)) == 0) continue;
    const SelTask& t = tasks[x];
    o[0] = 1; o[1] = (long long)(t.rd - dreads); o[2] = (long long)(t.tx - dtext); o[3] = t.gslot; o[4] = t.rl; o[5] = t.roff; o[6] = t.rlen; o[7] = t.tlen1; o[8] = t.fwd;
  }
  return (int)B.err;
}

// nt strip alignments in ONE launch of qp_sel_strip_kernel, four per wavefront in the order given: task[nt * 7] = {read offset, rl, roff, rlen, target
// offset, tlen1, fwd} into reads[nreads] / text[ntext] (characters); prm: {match, mismatch, gap open, gap extend}.  out[nt]: the scores.
int qp_sel_strip(int nt, const long long* task, const unsigned char* reads, long long nreads, const unsigned char* text, long long ntext, const int* prm, int* out) {
  if (nt < 1) return (int)hipErrorInvalidValue;
  for (int i = 0; i < nt; ++i) {
    const long long* t = task + 7 * i;
    if (!seq_ok(t[0], t[1], nreads) || t[2] < 0 || t[3] < 0 || t[2] + t[3] > t[1] || t[3] > QM_MAX_READ_LEN || !seq_ok(t[4], t[5], ntext) || t[5] > QM_MAX_READ_LEN + 48) return (int)hipErrorInvalidValue;
  }
  hipError_t e = hipSetDevice(0);
  if (e != hipSuccess) return (int)e;
  const size_t n = (size_t)nt;
  std::vector<unsigned char> hr(reads, reads + nreads), ht(text, text + ntext);
  hr.resize(hr.size() + 16, 0xA5); ht.resize(ht.size() + 16, 0xA5);
  ProbeBufs B;
  const unsigned char* dreads = B.put(hr.data(), hr.size()); const unsigned char* dtext = B.put(ht.data(), ht.size());
  std::vector<SelTask> tasks(n); std::vector<u64> order(n);
  for (size_t i = 0; i < n; ++i) {
    const long long* t = task + 7 * i;
    SelTask s; s.rd = dreads + t[0]; s.rl = (int)t[1]; s.roff = (int)t[2]; s.rlen = (int)t[3]; s.tx = dtext + t[4]; s.tlen1 = (int)t[5]; s.fwd = t[6] ? 1 : 0; s.gslot = (int)i;
    tasks[i] = s; order[i] = (u64)i;
  }
  const u64 ntasks2 = (u64)n;
  SelTask* dtasks = B.put(tasks.data(), n); u64* dorder = B.put(order.data(), n); u64* dnt = B.put(&ntasks2, 1);
  int* dtsc = B.fill<int>(n, 0x5A);
  if (B.err != hipSuccess) return (int)B.err;
  SelBatch A; memset(&A, 0, sizeof(A));
  A.seq1 = dreads; A.seq2 = dreads; A.text = dtext; A.tasks = dtasks; A.torder2 = dorder; A.ntasks2 = dnt; A.tsc = dtsc;
  A.match = prm[0]; A.mismatch = prm[1]; A.gap_open = prm[2]; A.gap_extend = prm[3];
  hipLaunchKernelGGL(qp_sel_strip_kernel, dim3(blocks_two_trips(nt, 16)), dim3(256), 0, 0, A);
  B.sync();
  B.get(out, dtsc, n);
  return (int)B.err;
}

}  // extern "C"
