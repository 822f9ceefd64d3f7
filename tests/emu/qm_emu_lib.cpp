// tests/emu/qm_emu_lib.cpp -- TEST-ONLY lane emulation of the library-type sweep: the driver of rapmap_amd/csrc/qm_lib_host.inl (and
// of qm_eqc_host.inl, which it hands its lists to) and the device code of qm_lib.inl, compiled with -DQM_EMU (an LV<T> is a 64-entry
// array, QM_LANES a loop, a launch a loop over the wavefronts: qm_exec.h).  What is here is a C face over the driver's object.  One
// wavefront after the other, one lane after the other: this checks the driver and the logic of the sweep -- codes, ballots, the
// scan's use, the compaction, the unit offsets, the parts of host arrays, the grid's cap --, not the atomics.  A sweep's scratch and its lists are handed over
// filled with 0xA5: the sweep must write what it reads.
#define QM_EMU
#include "../../rapmap_amd/csrc/qm_wave.h"
using namespace qm;
#include "../../rapmap_amd/csrc/qm_eqc_host.inl"
#include "../../rapmap_amd/csrc/qm_lib_host.inl"

static int emu_lib_open(qm_lib& L, u32 mask, int max_blocks, const u64* ctr, const LibSrc& S) {
  L.mask = mask; L.maxBlocks = max_blocks;
  int rc = lib_open(&L);
  if (rc) return rc;
  memcpy(L.d_ctr.p, ctr, LIB_WORDS * sizeof(u64));
  const long long hw = qx::waves_of(S.nh);
  L.d_keepMask.ensure(hw + 1); L.d_keepCnt.ensure(hw + 1); L.d_waveBase.ensure(hw + 1); L.d_outTids.ensure(std::max<long long>(S.nh, 1)); L.d_newOff.ensure(S.n + 1);
  memset(L.d_keepMask.p, 0xA5, (size_t)(hw + 1) * 8); memset(L.d_keepCnt.p, 0xA5, (size_t)(hw + 1) * 4); memset(L.d_waveBase.p, 0xA5, (size_t)(hw + 1) * 8);
  memset(L.d_outTids.p, 0xA5, (size_t)std::max<long long>(S.nh, 1) * 4); memset(L.d_newOff.p, 0xA5, (size_t)(S.n + 1) * 8);
  return QM_OK;
}

extern "C" {

int qe_lib_grid(long long lanes, int max_blocks) { return qmk_lib_grid(lanes, 256, max_blocks); }

// qm_lib_add_hits (new_off null) / qm_lib_compact_hits over the host arrays, in parts of at most max_units units and max_hits hits, into
// ctr[32] (added to; written back whatever the outcome).  new_off: n + 1 entries, out_tids: room for every hit.  hits may be null when no
// unit has a hit.  *sweeps: the sweeps it took.  Returns a QM_* code.
int qe_lib_add(long long n, const int64_t* off, const qm_hit* hits, u32 mask, int max_blocks, long long max_units, long long max_hits, u64* ctr,
               int64_t* new_off, u32* out_tids, long long* sweeps) {
  if (!mask || (mask & ~LIB_ALL_CODES)) return QM_E_ARG;
  const long long nh = n > 0 && off && off[n] > off[0] ? off[n] - off[0] : 0;
  qm_lib L;
  int rc = emu_lib_open(L, mask, max_blocks, ctr, LibSrc{nullptr, 0, nullptr, n > 0 ? n : 0, nh});
  if (!rc) rc = lib_add_host(&L, "qe_lib_add", n, off, hits, new_off, out_tids, max_units, max_hits);
  memcpy(ctr, L.d_ctr.p, LIB_WORDS * sizeof(u64));
  *sweeps = L.sweeps;
  return rc;
}

// qm_eqc_add_lib's fold of n units into a fresh table; the tallies into ctr[32].  out_off needs room for n + 2 entries, out_tids for
// off[n] + 1 words, out_counts for n + 1.  Returns the number of classes, or a QM_* code (negative).
long long qe_lib_eqc(long long n, const long long* off, const unsigned char* hits, int stride, u32 mask, int max_blocks, u64* ctr,
                     int64_t* out_off, u32* out_tids, uint64_t* out_counts) {
  if (!mask || (mask & ~LIB_ALL_CODES)) return QM_E_ARG;
  const LibSrc S{hits, stride, off, n, n > 0 ? off[n] : 0};
  qm_lib L; qm_eqc t;
  t.longMin = 4;
  int rc = emu_lib_open(L, mask, max_blocks, ctr, S);
  if (!rc) rc = eqc_open(&t, 16, 64);
  if (!rc) rc = lib_eqc_fold(&L, &t, S, t.stream);
  if (rc) return rc;
  memcpy(ctr, L.d_ctr.p, LIB_WORDS * sizeof(u64));
  if ((rc = eqc_fetch(&t, out_off, out_tids, out_counts))) return rc;
  return (long long)t.h[EQC_SC_CLASSES];
}

}  // extern "C"
