// qm_grid.h -- the grid of a persistent kernel: plain arithmetic, no HIP (tests/test_launch_grid.py compiles it with g++).
//
// Every stage-A kernel is a persistent grid whose waves stride over the work, in four-wave workgroups (the two headline kernels: in
// workgroups of one wave, see "the two headline kernels" below; their grids are counted in four-wave units all the same).  Launched with exactly the
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
//     (both: wave_grid -- 4 / QM_WG_WAVES workgroups of QM_WG_WAVES waves (default 1) per unit; resident: resident_quads_per_cu, the
//      occupancy query in workgroups x QM_WG_WAVES / 4 -- 32 one-wave workgroups per CU on gfx950 for both; runs of QM_WAVE_RUN trips
//      (default 8; 1, 2, 4, 8) per wave, fewer while the batch has not num_cu x 4 x resident runs of them)
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

// ---- the two headline kernels (qm_lean_kernel, qm_duo_kernel): workgroups of QM_WG_WAVES waves, runs of neighbouring trips per wave.
//
// The grid is still counted in units of four waves (grid_blocks, and QM_BLOCKS_PER_CU / the oversubscription knobs with it): a launch
// has 4 x grid_blocks(..) WAVES, in workgroups of QM_WG_WAVES (1, 2 or 4; a compile-time choice, because a block's LDS slabs are).
// Wave gw of nw takes RUNS gw, gw + nw, .. of R = 1 << rs consecutive trips (pairs, iterations) and maps each run's trips in order:
// neighbouring pairs' offsets and characters share sectors, and the wave that fetched a sector is the one that asks for it again.
// Static and deterministic; R = 1 is the strided order gw, gw + nw, ..  R comes from QM_WAVE_RUN (wave_run) and shrinks until the batch
// has at least as many runs as waves can be resident (run_shift), so that a small batch still fills the device.
#ifndef QM_WG_WAVES
#define QM_WG_WAVES 1
#endif
#if defined(__HIPCC__) && !defined(QM_EMU)
#define QM_GRID_FN __host__ __device__ inline
#else
#define QM_GRID_FN inline
#endif
constexpr int WAVE_RUN_MAX = 8;            // the longest run: the kernels stage a run's offsets in LDS (DuoMem / LeanMem::orun)
constexpr int WAVE_RUN_DEFAULT = 8;

// R as asked for: QM_WAVE_RUN = 1, 2, 4 or 8 (anything else: the default)
inline int wave_run() {
  static const int r = [] { const char* e = getenv("QM_WAVE_RUN"); const int v = e ? atoi(e) : 0; return v == 1 || v == 2 || v == 4 || v == 8 ? v : WAVE_RUN_DEFAULT; }();
  return r;
}
// blocks of wg_waves waves for a grid of `quads` four-wave units
inline int wave_blocks(int quads, int wg_waves) { return quads * (4 / wg_waves); }
// runs of 1 << rs trips that `trips` trips make (the last one may be short)
QM_GRID_FN long long run_count(long long trips, int rs) { return (trips + (1LL << rs) - 1) >> rs; }
// log2 of the run length of a batch: the largest power of two up to `want` that leaves at least resident_waves runs; 0 when none does
inline int run_shift(long long trips, long long resident_waves, int want) {
  int rs = 0;
  while ((2 << rs) <= want && (2 << rs) <= WAVE_RUN_MAX && run_count(trips, rs + 1) >= resident_waves) ++rs;
  return rs;
}
// a headline kernel's launch over `trips` trips: workgroups of QM_WG_WAVES waves (4 x grid_blocks(..) waves in all) and log2 of the run
// length; quads_per_cu: resident four-wave units per CU (resident_quads_per_cu, qm_device.h)
struct WaveGrid { int blocks, rs; };
inline WaveGrid wave_grid(long long trips, int num_cu, int quads_per_cu, int oversub) {
  const WaveGrid g = {wave_blocks(grid_blocks(trips, num_cu, quads_per_cu, oversub), QM_WG_WAVES), run_shift(trips, 4LL * num_cu * quads_per_cu, wave_run())};
  return g;
}
// the t-th trip of wave gw of nw; at or beyond the number of trips of the batch: the wave is through (a wave's trips ascend)
QM_GRID_FN long long run_trip(long long t, int gw, int nw, int rs) { return ((((t >> rs) * nw) + gw) << rs) + (t & ((1LL << rs) - 1)); }
// trip `it` (< trips) is the last one of its run
QM_GRID_FN int run_ends(int it, int trips, int rs) { return (it + 1 >= trips || ((it + 1) & ((1 << rs) - 1)) == 0) ? 1 : 0; }
// the first trip of the run `ahead` runs of the same wave behind the run of trip `it`; `trips` when the batch has no such run
QM_GRID_FN int run_ahead(int it, int trips, int nw, int rs, int ahead) {
  const unsigned n = ((unsigned)(it >> rs) + (unsigned)ahead * (unsigned)nw) << rs;   // (below 2^32: trips < 2^31, runs of at most eight, waves < 2^20)
  return n < (unsigned)trips ? (int)n : trips;
}
// the trip that wave maps behind `it`; `trips` when there is none
QM_GRID_FN int run_next(int it, int trips, int nw, int rs) { return run_ends(it, trips, rs) ? run_ahead(it, trips, nw, rs, 1) : it + 1; }

// the sweeps of the estimation objects (qm_fld.inl, qm_lib.inl, qm_gcb.inl, qm_sqb.inl, qm_psb.inl), one lane per unit, hit, window start or text position: the workgroups that are resident at
// once (FLD_ / LIB_ / GCB_ / SQB_ / PSB_*_BLOCKS_PER_CU, no query), fewer when the lanes do not fill them, at most max_blocks when that is not 0
inline int sweep_grid(long long lanes, int num_cu, int resident_per_cu, int max_blocks) {
  const int g = grid_blocks((lanes + 63) / 64, num_cu > 0 ? num_cu : 1, resident_per_cu, 1);
  return max_blocks > 0 && g > max_blocks ? max_blocks : g;
}

}  // namespace qm
