// tests/emu/qm_emu_lib.cpp -- TEST-ONLY lane emulation of the library-type sweep: the driver of rapmap_amd/csrc/qm_lib_host.inl (and
// of qm_eqc_host.inl, which it hands its lists to) and the device code of qm_lib.inl, compiled with -DQM_EMU (an LV<T> is a 64-entry
// array, QM_LANES a loop, a launch a loop over the wavefronts: qm_exec.h).  What is here is a C face over the driver's object.  One
// wavefront after the other, one lane after the other: this checks the driver and the logic of the sweep -- codes, ballots, the
// scan's use, the compaction, the unit offsets, the grid's cap --, not the atomics.  A sweep's scratch and its lists are handed over
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

// Sweeps n units (off[0] = 0) into ctr[32] (added to).  new_off (n + 1 entries) / out_tids (room for off[n]) not null: the filtered
// lists as well.  hits may be null when no unit has a hit.  Returns a QM_* code.
int qe_lib_sweep(long long n, const long long* off, const unsigned char* hits, int stride, u32 mask, int max_blocks, u64* ctr, long long* new_off, u32* out_tids) {
  if (!mask || (mask & ~LIB_ALL_CODES)) return QM_E_ARG;
  if (n <= 0) return QM_OK;
  const LibSrc S{hits, stride, off, n, off[n]};
  qm_lib L;
  int rc = emu_lib_open(L, mask, max_blocks, ctr, S);
  if (!rc) rc = lib_sweep(&L, S, new_off != nullptr, L.stream);
  if (rc) return rc;
  memcpy(ctr, L.d_ctr.p, LIB_WORDS * sizeof(u64));
  if (new_off) {
    memcpy(new_off, L.d_newOff.p, (size_t)(n + 1) * 8);
    if (new_off[n] < 0 || new_off[n] > off[n]) return QM_E_STATE;
    memcpy(out_tids, L.d_outTids.p, (size_t)new_off[n] * 4);
  }
  return QM_OK;
}

// qm_eqc_add_lib's fold of n units into a fresh table; the tallies into ctr[32].  out_off needs room for n + 2 entries, out_tids for
// off[n] + 1 words, out_counts for n + 1.  Returns the number of classes, or a QM_* code (negative).
long long qe_lib_eqc(long long n, const long long* off, const unsigned char* hits, int stride, u32 mask, int max_blocks, u64* ctr,
                     long long* out_off, u32* out_tids, u64* out_counts) {
  if (!mask || (mask & ~LIB_ALL_CODES)) return QM_E_ARG;
  const LibSrc S{hits, stride, off, n, n > 0 ? off[n] : 0};
  qm_lib L; qm_eqc t;
  t.longMin = 4;
  int rc = emu_lib_open(L, mask, max_blocks, ctr, S);
  if (!rc) rc = eqc_open(&t, 16, 64);
  if (!rc) rc = lib_eqc_fold(&L, &t, S, t.stream);
  if (rc) return rc;
  memcpy(ctr, L.d_ctr.p, LIB_WORDS * sizeof(u64));
  const EqcTable& T = t.T;
  std::vector<size_t> order;
  for (size_t s = 0; s <= T.mask; ++s) if (T.key[s]) order.push_back(s);
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    return std::lexicographical_compare(T.pool + T.loff[a], T.pool + T.loff[a] + T.llen[a], T.pool + T.loff[b], T.pool + T.loff[b] + T.llen[b]);
  });
  long long o = 0;
  for (size_t i = 0; i < order.size(); ++i) {
    const size_t s = order[i];
    out_off[i] = o; memcpy(out_tids + o, T.pool + T.loff[s], (size_t)T.llen[s] * 4); out_counts[i] = T.count[s]; o += T.llen[s];
  }
  out_off[order.size()] = o;
  return (long long)order.size();
}

}  // extern "C"
