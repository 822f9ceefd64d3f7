// qm_grid.h -- the grid of a persistent kernel: plain arithmetic, no HIP (tests/test_launch_grid.py compiles it with g++).
//
// Every stage-A kernel is a persistent grid of four-wave workgroups whose waves stride over the work.  Launched with exactly the
// blocks that are resident at once, the work is divided statically and the launch lasts as long as its slowest wave (13 % longer
// than the average one on config 2); launched with `oversub` times that many, the hardware hands the blocks out as slots free up:
// 41.6 -> 36.1 ms at 4 (profiles/r04/grid_oversub.txt; 8: the same).  So
//
//   blocks = max(1, min(blocks the work needs, num_cu x resident blocks per CU x oversub))
//
// and this table says what each kernel puts in.  resident: resident_per_cu (qm_device.h) -- the occupancy query of the chosen
// instantiation, the fallback where the query fails; "knob": QM_BLOCKS_PER_CU may lower it.  G = QM_GRID_OVERSUB (grid_oversub,
// default 4), P = QM_GRID_OVERSUB_PH (grid_oversub_ph: default 12, or G where only QM_GRID_OVERSUB is set).
//
//   kernel                      work, four units to a block   fallback   knob  oversub
//   qm_read_kernel<NS, WPS, F>  the caller's grid (blocks)    WPS        yes   F & QM_F_PH ? P : G
//   qm_lean_kernel              lean_iters(nreads, WIDE)      8          yes   NQ ? 1 : PH ? P : SEL ? G : 2 G
//   qm_duo_kernel               pair_iters(nreads)            8          yes   QM_DUO_OVERSUB if set, else PH ? P : 2 G
//   qm_h2m_kernel<0 / SEL>      the caller's grid (blocks)    2          no    1
//   qm_h2m_pack_kernel          the caller's grid (blocks)    2          no    G
//   qm_h2m_packw_kernel         the caller's grid (blocks)    1          no    G
//   map_grid                    reads                         nominal 8  no    the compact -p image ? P : G
//   resident_grid               reads                         nominal 8  no    1
//   fld_wave (qx::sweep)        sweep_grid: units / 64        8 (fixed)  no    1, then at most the caller's max_blocks
//   lib_classify_wave (sweep)   sweep_grid: hits / 64         8 (fixed)  no    1, then at most the caller's max_blocks
//   lib_units_wave (sweep)      sweep_grid: units / 64        8 (fixed)  no    1, then at most the caller's max_blocks
//   gcb_obs_wave (sweep)        sweep_grid: units / 64        8 (fixed)  no    1, then at most the caller's max_blocks
//   gcb_expect_wave (sweep)     sweep_grid: tiles of 64       8 (fixed)  no    1, then at most the caller's max_blocks
//   sqb_obs_wave (sweep)        sweep_grid: units / 64        8 (fixed)  no    1, then at most the caller's max_blocks
//   sqb_expect_wave (sweep)     sweep_grid: tiles of 64       4 (fixed)  no    1, then at most the caller's max_blocks
//   sqb_efflen_wave (sweep)     sweep_grid: tiles of 64       4 (fixed)  no    1, then at most the caller's max_blocks
//   psb_obs_wave (sweep)        sweep_grid: units / 64        8 (fixed)  no    1, then at most the caller's max_blocks
//   psb_expect_wave (sweep)     sweep_grid: 20 n_txps / 64    8 (fixed)  no    1, then at most the caller's max_blocks
//   psb_efflen_wave (sweep)     sweep_grid: tiles of 64       4 (fixed)  no    1, then at most the caller's max_blocks
//
// The fixed figures of the sweeps with an LDS slab come from the compute unit's 160 KiB: sqb_obs_wave keeps 1 152 32-bit words per
// wavefront (18 KiB per workgroup: 8 workgroups are 144 KiB, and the CU's 32 wavefronts), sqb_expect_wave 1 152 64-bit accumulators
// and sqb_efflen_wave a ring of 1 152 doubles (36 KiB per workgroup: 4 workgroups are 144 KiB, 16 wavefronts).  psb_obs_wave keeps
// 200 32-bit words per wavefront (3 200 bytes per workgroup) and psb_expect_wave 200 64-bit accumulators (6 400 bytes per workgroup):
// 8 workgroups are 25 and 50 KiB, and the CU's 32 wavefronts; psb_efflen_wave is sqb_efflen_wave's walk and keeps its ring.
//
// map_grid is the host's plan for the general kernels (the "caller's grid" above, and what their scratch and the bump allocators' slack
// are sized by); resident_grid the one it falls back to when that scratch does not fit, and the size of the list kernels' -s scratch.
//
// (the lean kernel's 2 G: 455-466 -> 468-471 M pairs/s with the batch in two parts, whose launches are short enough for their tails to
// show -- its waves reserve list room in quarters of the general kernels', QM_LEAN_CHUNK; its N-aware pass over a queue of a few hundred
// thousand reads: the resident grid, so that a wave's prologue is paid for by more than two or three iterations.  The compact -p
// kernels -- BooPHF walked per lookup: reads differ more in work -- keep gaining up to twelve times the resident blocks: 181.9 /
// 185.5 / 187.4 / 189.1 / 189.0 M pairs/s at 4 / 6 / 8 / 12 / 16, profiles/r04/ph_oversub.txt.)
#pragma once
#include <cstdlib>

namespace qm {

constexpr int GRID_NOMINAL_PER_CU = 8;     // resident blocks per CU where the host plans a grid without asking a kernel

inline int grid_oversub() {
  static const int m = [] { const char* e = getenv("QM_GRID_OVERSUB"); return e && atoi(e) > 0 && atoi(e) <= 16 ? atoi(e) : 4; }();
  return m;
}
inline int grid_oversub_ph() {
  static const int m = [] { const char* e = getenv("QM_GRID_OVERSUB_PH"); return e && atoi(e) > 0 && atoi(e) <= 16 ? atoi(e) : (getenv("QM_GRID_OVERSUB") ? grid_oversub() : 12); }();
  return m;
}

// `blocks` workgroups asked for -> launched
inline int grid_clamp(long long blocks, int num_cu, int resident_per_cu, int oversub) {
  const long long cap = (long long)num_cu * resident_per_cu * oversub;
  const long long g = blocks < cap ? blocks : cap;
  return (int)(g > 0 ? g : 1);
}
// the same for `work` units, one per wave and trip: four to a block
inline int grid_blocks(long long work, int num_cu, int resident_per_cu, int oversub) { return grid_clamp((work + 3) / 4, num_cu, resident_per_cu, oversub); }

// trips of the lean kernel (two reads per wavefront; its wide edition: one) and of the pair kernel (a pair) over nreads reads
inline long long lean_iters(long long nreads, bool wide) { return wide ? nreads : (nreads + 1) >> 1; }
inline long long pair_iters(long long nreads) { return nreads >> 1; }

// the general kernels' grid over nreads reads as the host plans it (ph_compact: the compact -p image), and the one without
// oversubscription (kernels that own per-wave scratch in device memory: the list kernels)
inline int map_grid(long long nreads, int num_cu, bool ph_compact) { return grid_blocks(nreads, num_cu, GRID_NOMINAL_PER_CU, ph_compact ? grid_oversub_ph() : grid_oversub()); }
inline int resident_grid(long long nreads, int num_cu) { return grid_blocks(nreads, num_cu, GRID_NOMINAL_PER_CU, 1); }

// the sweeps of the estimation objects (qm_fld.inl, qm_lib.inl, qm_gcb.inl, qm_sqb.inl, qm_psb.inl), one lane per unit, hit, window start or text position: the workgroups that are resident at
// once (FLD_ / LIB_ / GCB_ / SQB_ / PSB_*_BLOCKS_PER_CU, no query), fewer when the lanes do not fill them, at most max_blocks when that is not 0
inline int sweep_grid(long long lanes, int num_cu, int resident_per_cu, int max_blocks) {
  const int g = grid_blocks((lanes + 63) / 64, num_cu > 0 ? num_cu : 1, resident_per_cu, 1);
  return max_blocks > 0 && g > max_blocks ? max_blocks : g;
}

}  // namespace qm
