// tests/emu/qm_emu_h2m.cpp -- TEST-ONLY lane emulation of the lean kernel's hits-to-mappings pass by itself: rapmap_amd/csrc/qm_lean.inl
// compiled with -DQM_EMU (an LV<T> is a 64-entry array, QM_LANES a loop).  The entry point fills a wave's suffix stash the way the walks
// of lean_iter leave it -- n entries, the rest of the 64 slots holding whatever they held (0xA5 here) -- and runs one edition of the pass:
// the dispatcher the kernels call (lean_h2m), the scalar-indexed loop (lean_h2m_loop) or the 8 x 8 tiles (lean_h2m_tiles, n <= 32).
#define QM_EMU
#include "../../rapmap_amd/csrc/qm_lean.inl"

#include <string.h>

using namespace qm;

extern "C" {

int qe_h2m_tile_lo(void) { return QM_H2M_TILE_LO; }
int qe_h2m_tile_hi(void) { return QM_H2M_TILE_HI; }

// which: 0 lean_h2m, 1 lean_h2m_loop, 2 lean_h2m_tiles (n <= 32), 3 its single-tile edition (n <= 8). stash: n x {tid, pos, qp, iv}.  Out, for all 64 lanes: elem, keep, slot.
// Returns the survivor count, -1 for a bad argument.
int qe_h2m(int which, int n, int m, int min_idx, int is_rc, const u32* stash, u64* elem, unsigned char* keep, int* slot) {
  if (n < 0 || n > QM_LEAN_SUF || m < 1 || m > QM_LEAN_MAXIV || min_idx < 0 || min_idx >= m) return -1;
  if (which == 2 && n > 32) return -1;
  LeanSuf suf[QM_LEAN_SUF];
  memset(suf, 0xA5, sizeof(suf));
  for (int i = 0; i < n; ++i) { suf[i].tid = stash[4 * i]; suf[i].pos = stash[4 * i + 1]; suf[i].qp = stash[4 * i + 2]; suf[i].iv = stash[4 * i + 3]; }
  LeanStrand S; S.n = m; S.sufN = n; S.minIdx = min_idx; S.minSpan = 0; S.cov = 0;
  LV<u64> e; LV<bool> k; LV<int> s;
  for (int l = 0; l < 64; ++l) { e.v[l] = 0x5A5A5A5A5A5A5A5AULL; k.v[l] = true; s.v[l] = -77; }   // (nothing of the caller's survives the pass)
  int cnt;
  if (which == 0) cnt = lean_h2m(suf, S, is_rc != 0, e, k, s);
  else if (which == 1) cnt = lean_h2m_loop(suf, S, is_rc != 0, e, k, s);
  else if (which == 2) cnt = lean_h2m_tiles<false>(suf, S, is_rc != 0, e, k, s);
  else if (which == 3 && n <= 8) cnt = lean_h2m_tiles<true>(suf, S, is_rc != 0, e, k, s);
  else return -1;
  for (int l = 0; l < 64; ++l) { elem[l] = e.v[l]; keep[l] = k.v[l] ? 1 : 0; slot[l] = s.v[l]; }
  return cnt;
}

}  // extern "C"
