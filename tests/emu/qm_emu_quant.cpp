// tests/emu/qm_emu_quant.cpp -- TEST-ONLY lane emulation of the abundance-estimation device code: rapmap_amd/csrc/qm_quant.inl compiled
// with -DQM_EMU (an LV<T> is a 64-entry array, QM_LANES a loop), driven the way qm_quant_host.inl drives the kernels: mark, scans,
// compact, sort, bounds, row statistics and queues, then per iteration a class launch and a transcript launch.  Host-side scans and a
// std::stable_sort stand in for rocPRIM.  One wavefront after the other, one lane after the other: this checks the logic of the
// structure build and of the two iteration bodies (and the order of their sums), not the atomics.
#define QM_EMU
#include "../../rapmap_amd/csrc/qm_quant.inl"

#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

using namespace qm;

namespace {
void scan(const std::vector<u32>& in, std::vector<long long>& out, long long n) {
  long long s = 0;
  for (long long i = 0; i < n; ++i) { out[(size_t)i] = s; s += in[(size_t)i]; }
}
long long waves_of(long long lanes) { return (lanes + 63) / 64; }
}  // namespace

extern "C" {

// The table: nc classes in canonical arrays (off, tids, cnt), laid out here as an EqcTable with unpublished slots between the
// published ones.  eff: nTxps numbers; alpha0: nTxps numbers or NULL (the uniform start).  out_alpha: nTxps numbers.
// stats: [0] classes [1] entries [2] present [3] longest label [4] longest list [5] queued labels [6] queued transcripts [7] iterations.
// Returns 0, or -1 when a label names a transcript >= nTxps (QM_E_ARG on the device).
int qe_quant_run(long long nc, const long long* off, const u32* tids, const u64* cnt, long long nTxps, const double* eff, const double* alpha0,
                 int max_iter, int check_every, double rel_tol, double min_alpha, double* out_alpha, double* out_rel, long long* stats) {
  const long long ne = off[nc], cap = 2 * nc + 5;
  std::vector<u64> key((size_t)cap, 0), count((size_t)cap, 0); std::vector<long long> loff((size_t)cap, 0); std::vector<u32> llen((size_t)cap, 0), pool((size_t)ne + 1);
  if (ne) memcpy(pool.data(), tids, (size_t)ne * 4);
  u64 total = 0;
  for (long long c = 0; c < nc; ++c) { const size_t s = (size_t)(2 * c + 1); key[s] = 1ULL << 63; count[s] = cnt[c]; loff[s] = off[c]; llen[s] = (u32)(off[c + 1] - off[c]); total += cnt[c]; }
  u64 scal[QNT_SC_WORDS] = {0};
  const long long nflag = std::max(cap, nTxps) + 1;
  std::vector<u32> flag((size_t)nflag), len((size_t)cap + 1), pairTid((size_t)ne + 1), pairCls((size_t)ne + 1), sortedTid((size_t)ne + 1), clab((size_t)ne + 1), tcls((size_t)ne + 1);
  std::vector<long long> cidx((size_t)nflag), lofs((size_t)cap + 1), coff((size_t)nc + 1, 0), toff((size_t)nTxps + 1, 0), qCls, qTxp;
  std::vector<double> dcnt((size_t)nc + 1), single((size_t)nTxps + 1, 0.0), w((size_t)nTxps + 1, 0.0), r((size_t)nc + 1, 0.0), alpha[2];
  alpha[0].assign((size_t)nTxps + 1, 0.0); alpha[1].assign((size_t)nTxps + 1, 0.0);
  QuantBuild B{};
  B.key = key.data(); B.llen = llen.data(); B.loff = loff.data(); B.count = count.data(); B.pool = pool.data(); B.cap = cap;
  B.flag = flag.data(); B.len = len.data(); B.cidx = cidx.data(); B.lofs = lofs.data(); B.nTxps = (u64)nTxps; B.scal = scal;
  B.coff = coff.data(); B.clab = clab.data(); B.cnt = dcnt.data(); B.pairTid = pairTid.data(); B.pairCls = pairCls.data(); B.single = single.data();
  for (long long wv = 0; wv < waves_of(cap + 1); ++wv) quant_mark_wave(B, wv);
  scan(flag, cidx, cap + 1); scan(len, lofs, cap + 1);
  if (cidx[(size_t)cap] != nc || lofs[(size_t)cap] != ne) return -7;
  long long nqCls = 0, nqTxp = 0;
  if (nc > 0) {
    for (long long wv = 0; wv < waves_of(cap + 1); ++wv) quant_compact_wave(B, wv);
    if (scal[QNT_SC_BAD_TID]) return -1;
    std::vector<long long> perm((size_t)ne);
    std::iota(perm.begin(), perm.end(), 0LL);
    std::stable_sort(perm.begin(), perm.end(), [&](long long a, long long b) { return pairTid[(size_t)a] < pairTid[(size_t)b]; });
    for (long long i = 0; i < ne; ++i) { sortedTid[(size_t)i] = pairTid[(size_t)perm[(size_t)i]]; tcls[(size_t)i] = pairCls[(size_t)perm[(size_t)i]]; }
    for (long long wv = 0; wv < waves_of(nTxps + 1); ++wv) quant_bounds_wave(sortedTid.data(), ne, nTxps, toff.data(), wv);
    for (long long wv = 0; wv < waves_of(nc + 1); ++wv) quant_rowstat_wave(coff.data(), nc, flag.data(), scal, QNT_SC_MAX_LABEL, 0, wv);
    scan(flag, cidx, nc + 1); nqCls = cidx[(size_t)nc]; qCls.assign((size_t)nqCls + 1, -1);
    for (long long wv = 0; wv < waves_of(nc); ++wv) quant_queue_wave(flag.data(), cidx.data(), nc, qCls.data(), wv);
    for (long long wv = 0; wv < waves_of(nTxps + 1); ++wv) quant_rowstat_wave(toff.data(), nTxps, flag.data(), scal, QNT_SC_MAX_LIST, 1, wv);
    scan(flag, cidx, nTxps + 1); nqTxp = cidx[(size_t)nTxps]; qTxp.assign((size_t)nqTxp + 1, -1);
    for (long long wv = 0; wv < waves_of(nTxps); ++wv) quant_queue_wave(flag.data(), cidx.data(), nTxps, qTxp.data(), wv);
  }
  const long long present = (long long)scal[QNT_SC_PRESENT];
  int cur = 0;
  if (alpha0) { if (nTxps) memcpy(alpha[0].data(), alpha0, (size_t)nTxps * 8); }
  else if (present) for (long long wv = 0; wv < waves_of(nTxps); ++wv) quant_start_wave(toff.data(), nTxps, (double)total / (double)present, alpha[0].data(), wv);
  int it = 0; double rel = -1.0;
  if (nc > 0 && max_iter > 0) {
    for (long long wv = 0; wv < waves_of(nTxps); ++wv) quant_weights_wave(alpha[cur].data(), eff, nTxps, w.data(), wv);
    QuantState Q{};
    Q.cls = QuantCsr{coff.data(), clab.data(), nc, qCls.data(), nqCls};
    Q.txp = QuantCsr{toff.data(), tcls.data(), nTxps, qTxp.data(), nqTxp};
    Q.cnt = dcnt.data(); Q.eff = eff; Q.single = single.data(); Q.w = w.data(); Q.r = r.data(); Q.scal = scal; Q.minAlpha = min_alpha;
    while (it < max_iter) {
      const bool check = rel_tol > 0 && (it + 1) % check_every == 0;
      Q.alpha = alpha[cur].data(); Q.alphaNew = alpha[cur ^ 1].data(); Q.check = check ? 1 : 0;
      if (check) scal[QNT_SC_REL] = 0;
      for (long long wv = 0; wv < quant_side_waves(Q.cls); ++wv) quant_class_wave(Q, wv);
      for (long long wv = 0; wv < quant_side_waves(Q.txp); ++wv) quant_txp_wave(Q, wv);
      cur ^= 1; ++it;
      if (check) { memcpy(&rel, &scal[QNT_SC_REL], 8); if (rel < rel_tol) break; }
    }
  }
  if (nTxps) memcpy(out_alpha, alpha[cur].data(), (size_t)nTxps * 8);
  *out_rel = rel;
  stats[0] = nc; stats[1] = ne; stats[2] = present; stats[3] = (long long)scal[QNT_SC_MAX_LABEL]; stats[4] = (long long)scal[QNT_SC_MAX_LIST];
  stats[5] = nqCls; stats[6] = nqTxp; stats[7] = it;
  return 0;
}

}  // extern "C"
