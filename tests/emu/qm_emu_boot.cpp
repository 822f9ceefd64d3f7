// tests/emu/qm_emu_boot.cpp -- TEST-ONLY lane emulation of the bootstrap device code: rapmap_amd/csrc/qm_boot.inl (and the structure
// build of qm_quant.inl under it) compiled with -DQM_EMU, driven the way qm_quant_host.inl and qm_boot_host.inl drive the kernels.
// Host-side scans and a std::stable_sort stand in for rocPRIM.  One wavefront after the other, one lane after the other: this checks
// the draw, the logic of the batched iteration bodies, the order of their sums and the per-replicate stop -- not the atomics.
#define QM_EMU
#include "../../rapmap_amd/csrc/qm_boot.inl"

#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

using namespace qm;

namespace {
long long waves_of(long long lanes) { return (lanes + 63) / 64; }
void scan(const std::vector<u32>& in, std::vector<long long>& out, long long n) {
  long long s = 0;
  for (long long i = 0; i < n; ++i) { out[(size_t)i] = s; s += in[(size_t)i]; }
}

struct Boot {
  // the quant object's part: the graph in snapshot order (here: the order of the canonical arrays), effective lengths
  long long nc = 0, ne = 0, nT = 0, present = 0; u64 total = 0;
  std::vector<long long> coff, toff, qCls, qTxp; std::vector<u32> clab, tcls; std::vector<double> dcnt, eff;
  long long nqCls = 0, nqTxp = 0;
  // the boot object's
  long long nReps = 0, Bp = 0; u64 N = 0; bool haveCounts = false; int aggregate = 0;
  std::vector<u64> cnt0, cum, cnt, rel, scal; std::vector<double> single, w, r, alpha, lastRel; std::vector<u32> done; std::vector<int> iters;
  BootBook book() { return BootBook{done.data(), rel.data(), iters.data(), lastRel.data(), scal.data()}; }
};

// the structure build of qm_emu_quant.cpp, kept to what the bootstrap borrows; -1: a label names a transcript >= nTxps
int build_graph(Boot& B, long long nc, const long long* off, const u32* tids, const u64* cnt, long long nTxps) {
  const long long ne = off[nc], cap = 2 * nc + 5;
  std::vector<u64> key((size_t)cap, 0), count((size_t)cap, 0); std::vector<long long> loff((size_t)cap, 0); std::vector<u32> llen((size_t)cap, 0), pool((size_t)ne + 1);
  if (ne) memcpy(pool.data(), tids, (size_t)ne * 4);
  for (long long c = 0; c < nc; ++c) { const size_t s = (size_t)(2 * c + 1); key[s] = 1ULL << 63; count[s] = cnt[c]; loff[s] = off[c]; llen[s] = (u32)(off[c + 1] - off[c]); B.total += cnt[c]; }
  u64 scal[QNT_SC_WORDS] = {0};
  const long long nflag = std::max(cap, nTxps) + 1;
  std::vector<u32> flag((size_t)nflag), len((size_t)cap + 1), pairTid((size_t)ne + 1), pairCls((size_t)ne + 1), sortedTid((size_t)ne + 1);
  std::vector<long long> cidx((size_t)nflag), lofs((size_t)cap + 1);
  std::vector<double> single((size_t)nTxps + 1, 0.0);
  B.nc = nc; B.ne = ne; B.nT = nTxps;
  B.coff.assign((size_t)nc + 1, 0); B.toff.assign((size_t)nTxps + 1, 0); B.clab.assign((size_t)ne + 1, 0); B.tcls.assign((size_t)ne + 1, 0); B.dcnt.assign((size_t)nc + 1, 0.0);
  QuantBuild Q{};
  Q.key = key.data(); Q.llen = llen.data(); Q.loff = loff.data(); Q.count = count.data(); Q.pool = pool.data(); Q.cap = cap;
  Q.flag = flag.data(); Q.len = len.data(); Q.cidx = cidx.data(); Q.lofs = lofs.data(); Q.nTxps = (u64)nTxps; Q.scal = scal;
  Q.coff = B.coff.data(); Q.clab = B.clab.data(); Q.cnt = B.dcnt.data(); Q.pairTid = pairTid.data(); Q.pairCls = pairCls.data(); Q.single = single.data();
  for (long long wv = 0; wv < waves_of(cap + 1); ++wv) quant_mark_wave(Q, wv);
  scan(flag, cidx, cap + 1); scan(len, lofs, cap + 1);
  if (cidx[(size_t)cap] != nc || lofs[(size_t)cap] != ne) return -7;
  if (nc == 0) return 0;
  for (long long wv = 0; wv < waves_of(cap + 1); ++wv) quant_compact_wave(Q, wv);
  if (scal[QNT_SC_BAD_TID]) return -1;
  std::vector<long long> perm((size_t)ne);
  std::iota(perm.begin(), perm.end(), 0LL);
  std::stable_sort(perm.begin(), perm.end(), [&](long long a, long long b) { return pairTid[(size_t)a] < pairTid[(size_t)b]; });
  for (long long i = 0; i < ne; ++i) { sortedTid[(size_t)i] = pairTid[(size_t)perm[(size_t)i]]; B.tcls[(size_t)i] = pairCls[(size_t)perm[(size_t)i]]; }
  for (long long wv = 0; wv < waves_of(nTxps + 1); ++wv) quant_bounds_wave(sortedTid.data(), ne, nTxps, B.toff.data(), wv);
  for (long long wv = 0; wv < waves_of(nTxps + 1); ++wv) quant_rowstat_wave(B.toff.data(), nTxps, flag.data(), scal, QNT_SC_MAX_LIST, 1, wv);
  B.present = (long long)scal[QNT_SC_PRESENT];
  return 0;
}

void side_queue(const std::vector<long long>& off, long long n, std::vector<long long>& queue, long long* nq) {
  std::vector<u32> flag((size_t)n + 1); std::vector<long long> pos((size_t)n + 1);
  for (long long wv = 0; wv < waves_of(n + 1); ++wv) boot_rowflag_wave(off.data(), n, flag.data(), wv);
  scan(flag, pos, n + 1);
  *nq = pos[(size_t)n]; queue.assign((size_t)*nq + 1, -1);
  for (long long wv = 0; wv < waves_of(n); ++wv) quant_queue_wave(flag.data(), pos.data(), n, queue.data(), wv);
}

void restart(Boot& B, long long s0, long long ns, u64 total) {
  const double value = B.present > 0 ? (double)total / (double)B.present : 0.0;
  for (long long tile = 0; tile < B.Bp / BOOT_TILE; ++tile)
    for (long long wv = 0; wv < boot_row_waves(B.nT); ++wv) boot_start_wave(B.toff.data(), B.eff.data(), B.nT, value, B.alpha.data(), B.w.data(), B.Bp, s0, ns, wv, tile);
  BootBook K = B.book();
  for (long long wv = 0; wv < waves_of(ns); ++wv) boot_reset_wave(K, s0, ns, wv);
}
}  // namespace

extern "C" {

// The table: nc classes in canonical arrays (off, tids, cnt); the snapshot order is theirs.  eff: nTxps numbers.  *err: 0, or -1 when a
// label names a transcript >= nTxps.  aggregate: the resample's per-wavefront aggregation on or off (the counts do not depend on it).
void* qe_boot_create(long long nc, const long long* off, const u32* tids, const u64* cnt, long long nTxps, const double* eff, int n_reps, int aggregate, int* err) {
  Boot* B = new Boot();
  *err = build_graph(*B, nc, off, tids, cnt, nTxps);
  if (*err) { delete B; return nullptr; }
  B->eff.assign(eff, eff + nTxps); B->eff.push_back(1.0);
  B->nReps = n_reps; B->Bp = boot_padded(n_reps); B->aggregate = aggregate;
  const size_t perC = (size_t)(std::max<long long>(nc, 1) * B->Bp), perT = (size_t)(std::max<long long>(nTxps, 1) * B->Bp);
  B->cnt0.assign((size_t)nc + 1, 0); B->cum.assign((size_t)nc + 1, 0); B->cnt.assign(perC, 0); B->r.assign(perC, 0.0);
  B->single.assign(perT, 0.0); B->w.assign(perT, 0.0); B->alpha.assign(perT, 0.0);
  B->rel.assign((size_t)B->Bp, 0); B->lastRel.assign((size_t)B->Bp, -1.0); B->done.assign((size_t)B->Bp, 1u); B->iters.assign((size_t)B->Bp, 0); B->scal.assign(BOOT_SC_WORDS, 0);
  for (int i = 0; i < n_reps; ++i) B->done[(size_t)i] = 0;
  for (long long wv = 0; wv < waves_of(nc + 1); ++wv) boot_counts_wave(B->dcnt.data(), nc, B->cnt0.data(), wv);
  u64 s = 0;
  for (long long c = 0; c <= nc; ++c) { B->cum[(size_t)c] = s; s += B->cnt0[(size_t)c]; }
  B->N = B->cum[(size_t)nc];
  if (B->N != B->total) { *err = -7; delete B; return nullptr; }
  if (nc > 0) { side_queue(B->coff, nc, B->qCls, &B->nqCls); side_queue(B->toff, nTxps, B->qTxp, &B->nqTxp); }
  return B;
}
void qe_boot_destroy(void* h) { delete (Boot*)h; }

// stats: [0] classes [1] entries [2] present [3] N [4] queued labels [5] queued transcripts
void qe_boot_info(void* h, long long* stats) {
  Boot& B = *(Boot*)h;
  stats[0] = B.nc; stats[1] = B.ne; stats[2] = B.present; stats[3] = (long long)B.N; stats[4] = B.nqCls; stats[5] = B.nqTxp;
}
void qe_boot_classes(void* h, long long* off, u32* tids, u64* cnt) {
  Boot& B = *(Boot*)h;
  memcpy(off, B.coff.data(), (size_t)(B.nc + 1) * 8);
  if (B.ne) memcpy(tids, B.clab.data(), (size_t)B.ne * 4);
  if (B.nc) memcpy(cnt, B.cnt0.data(), (size_t)B.nc * 8);
}

void qe_boot_resample(void* h, u64 seed, long long first_rep) {
  Boot& B = *(Boot*)h;
  if (B.nc > 0) {
    std::fill(B.cnt.begin(), B.cnt.end(), 0);
    BootDraw D{B.cum.data(), B.nc, B.N, seed, (u64)first_rep, B.cnt.data(), B.Bp, B.aggregate};
    const long long waves = (long long)(((B.N + 1) / 2 + 63) / 64);
    for (long long slot = 0; slot < B.nReps; ++slot) for (long long wv = 0; wv < waves; ++wv) boot_resample_wave(D, wv, slot);
    for (long long tile = 0; tile < B.Bp / BOOT_TILE; ++tile)
      for (long long wv = 0; wv < boot_row_waves(B.nc); ++wv) boot_single_wave(B.coff.data(), B.clab.data(), B.nc, B.cnt.data(), B.single.data(), B.Bp, wv, tile);
  }
  restart(B, 0, B.nReps, B.N);
  B.haveCounts = true;
}
int qe_boot_column(void* h, int rep, u64* col, int put) {
  Boot& B = *(Boot*)h;
  if (rep < 0 || rep >= B.nReps) return -1;
  for (long long wv = 0; wv < waves_of(B.nc); ++wv) boot_column_wave(B.coff.data(), B.clab.data(), B.nc, B.cnt.data(), B.single.data(), B.Bp, rep, col, put, wv);
  if (put) {
    u64 total = 0;
    for (long long c = 0; c < B.nc; ++c) total += col[c];
    restart(B, rep, 1, total);
    B.haveCounts = true;
  }
  return 0;
}

// -7: no counts yet.  launches: the class, transcript and mark launches of this run.
int qe_boot_run(void* h, int max_iter, int check_every, double rel_tol, double min_alpha, int* iterations, double* last_rel, long long* launches) {
  Boot& B = *(Boot*)h;
  if (!B.haveCounts) return -7;
  BootBook K = B.book();
  int it = 0; *launches = 0;
  for (long long wv = 0; wv < waves_of(B.nReps); ++wv) boot_begin_wave(K, B.nReps, wv);
  if (B.nc > 0 && max_iter > 0 && B.scal[BOOT_SC_DONE] < (u64)B.nReps) {
    BootState S{};
    S.cls = QuantCsr{B.coff.data(), B.clab.data(), B.nc, B.qCls.data(), B.nqCls};
    S.txp = QuantCsr{B.toff.data(), B.tcls.data(), B.nT, B.qTxp.data(), B.nqTxp};
    S.eff = B.eff.data(); S.cnt = B.cnt.data(); S.single = B.single.data(); S.w = B.w.data(); S.r = B.r.data(); S.alpha = B.alpha.data(); S.rel = B.rel.data(); S.done = B.done.data();
    S.Bp = B.Bp; S.minAlpha = min_alpha;
    while (it < max_iter) {
      const bool check = rel_tol > 0 && (it + 1) % check_every == 0;
      S.check = check ? 1 : 0;
      for (long long tile = 0; tile < B.Bp / BOOT_TILE; ++tile) for (long long wv = 0; wv < boot_side_waves(S.cls); ++wv) boot_class_wave(S, wv, tile);
      for (long long tile = 0; tile < B.Bp / BOOT_TILE; ++tile) for (long long wv = 0; wv < boot_side_waves(S.txp); ++wv) boot_txp_wave(S, wv, tile);
      ++it; *launches += 2;
      if (check) {
        for (long long wv = 0; wv < waves_of(B.nReps); ++wv) boot_mark_wave(K, B.nReps, it, rel_tol, wv);
        ++*launches;
        if (B.scal[BOOT_SC_DONE] >= (u64)B.nReps) break;
      }
    }
  }
  for (long long wv = 0; wv < waves_of(B.nReps); ++wv) boot_end_wave(K, B.nReps, it, wv);
  memcpy(iterations, B.iters.data(), (size_t)B.nReps * 4);
  memcpy(last_rel, B.lastRel.data(), (size_t)B.nReps * 8);
  return 0;
}

void qe_boot_fetch(void* h, double* out) {
  Boot& B = *(Boot*)h;
  for (long long slot = 0; slot < B.nReps; ++slot) for (long long wv = 0; wv < waves_of(B.nT); ++wv) boot_transpose_wave(B.alpha.data(), B.nT, B.Bp, out, wv, slot);
}

void qe_boot_philox(const u32* ctr, const u32* key, u32* out) { boot_philox(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], out); }

}  // extern "C"
