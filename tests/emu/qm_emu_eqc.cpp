// tests/emu/qm_emu_eqc.cpp -- TEST-ONLY lane emulation of the equivalence-class device code: rapmap_amd/csrc/qm_eqc.inl compiled
// with -DQM_EMU (an LV<T> is a 64-entry array, QM_LANES a loop), driven the way qm_eqc_host.inl drives the kernels: label launch,
// queue launch, rounds of probe / publish, a rebuild when slots or pool run out.  One wavefront after the other, one lane after
// the other: this checks the logic of the label and insert stages, not the atomics.
#define QM_EMU
#include "../../rapmap_amd/csrc/qm_eqc.inl"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace qm;

namespace {
struct Tab {
  std::vector<u64> key, claim, count; std::vector<long long> loff; std::vector<u32> llen, pool;
  EqcTable T;
  void init(u64 cap, u64 poolCap, u64* scal) {
    key.assign(cap, 0); claim.assign(cap, ~0ULL); count.assign(cap, 0); loff.assign(cap, 0); llen.assign(cap, 0); pool.assign(poolCap, 0);
    T.key = key.data(); T.claim = claim.data(); T.count = count.data(); T.loff = loff.data(); T.llen = llen.data(); T.pool = pool.data();
    T.mask = cap - 1; T.maxClasses = cap / 2; T.poolCap = poolCap; T.scal = scal;
  }
};
struct Emu {
  u64 scal[EQC_SC_WORDS] = {0};
  Tab* tab = nullptr;
  long long growths = 0, rounds = 0;
  int aggregate = 1;
  int insert(const EqcSet& S, bool mayGrow);
  int grow();
};
int Emu::grow() {
  Tab* old = tab;
  const u64 oldCap = old->T.mask + 1;
  const bool slots = scal[EQC_SC_SLOT_OVF] || scal[EQC_SC_FULL];
  Tab* nt = new Tab();
  nt->init(slots ? oldCap * 4 : oldCap, scal[EQC_SC_POOL_OVF] ? old->T.poolCap * 4 : old->T.poolCap, scal);
  for (int i = EQC_SC_FULL; i < EQC_SC_FULL + 6; ++i) scal[i] = 0;
  tab = nt;
  const EqcSet R{old->T.pool, old->T.loff, old->T.llen, old->T.key, old->T.count, (long long)oldCap};
  const int rc = insert(R, false);
  delete old;
  growths++;
  return rc;
}
int Emu::insert(const EqcSet& S, bool mayGrow) {
  std::vector<u64> q[2]; q[0].resize((size_t)S.n + 1); q[1].resize((size_t)S.n + 1);
  const u64* qin = nullptr; long long nin = S.n; int cur = 0;
  for (long long guard = 0; guard < (1 << 24); ++guard) {
    scal[EQC_SC_PEND] = scal[EQC_SC_FULL] = 0;
    for (long long w = 0; w < (nin + 63) / 64; ++w) eqc_probe_wave(tab->T, S, qin, nin, q[cur].data(), w, aggregate);
    rounds++;
    const long long pend = (long long)scal[EQC_SC_PEND];
    if (!pend) return 0;
    if (scal[EQC_SC_SLOT_OVF] || scal[EQC_SC_POOL_OVF] || scal[EQC_SC_FULL]) {
      if (!mayGrow) return -2;
      if (int rc = grow()) return rc;
      for (long long i = 0; i < pend; ++i) q[cur][(size_t)i] &= 0xffffffffULL;
    }
    else for (long long w = 0; w < (pend + 63) / 64; ++w) eqc_publish_wave(tab->T, S, q[cur].data(), pend, w);
    qin = q[cur].data(); nin = pend; cur ^= 1;
  }
  return -3;
}
}  // namespace

extern "C" {

// Folds `folds` times the n lists (tids at `stride` bytes) into a fresh table of `cap` slots (a power of two) and `pool_cap` pool
// words; out_off needs room for as many classes as there are lists (+ 1), out_tids for off[n] words.  long_cap: capacity of the
// long-unit queue (a smaller one than the units need is grown after the count, as on the device).
// stats: [0] growths [1] collision probes [2] long units [3] rounds.  Returns the number of classes, negative on an error.
long long qe_eqc_run(long long n, const long long* off, const unsigned char* tids, int stride, const u64* weights, int hash_bits, u64 cap, u64 pool_cap,
                     long long long_cap, int aggregate, int folds, long long* out_off, u32* out_tids, u64* out_counts, long long* stats) {
  Emu E; E.aggregate = aggregate;
  E.tab = new Tab(); E.tab->init(cap, pool_cap, E.scal);
  const long long nt = off[n];
  std::vector<u32> lab((size_t)nt + 1), len((size_t)n + 1); std::vector<u64> key((size_t)n + 1);
  std::vector<long long> longq((size_t)(long_cap > 0 ? long_cap : 1));
  std::vector<u32> slab(EQC_SLAB);
  long long longUnits = 0; int rc = 0;
  for (int f = 0; f < folds && !rc; ++f) {
    EqcSrc S{};
    S.tids = tids; S.stride = stride; S.off = off; S.n = n; S.lab = lab.data(); S.len = len.data(); S.key = key.data();
    S.scal = E.scal; S.keyMask = hash_bits ? ((1ULL << hash_bits) - 1) : ~0ULL;
    long long nl = 0;
    for (;;) {
      S.longq = longq.data(); S.longCap = (u64)longq.size();
      E.scal[EQC_SC_LONGQ] = 0;
      for (long long w = 0; w < (n + 64 / EQC_GROUP - 1) / (64 / EQC_GROUP); ++w) eqc_label_wave(S, w);
      nl = (long long)E.scal[EQC_SC_LONGQ];
      if (nl <= (long long)longq.size()) break;
      longq.assign((size_t)nl, -1);
    }
    for (long long w = 0; w < nl; ++w) eqc_label_queued(S, w, slab.data());
    longUnits += nl;
    const EqcSet set{S.lab, S.off, S.len, S.key, weights, n};
    rc = E.insert(set, true);
  }
  long long nc = rc;
  if (!rc) {
    const Tab& T = *E.tab;
    std::vector<size_t> order;
    for (size_t s = 0; s < T.key.size(); ++s) if (T.key[s]) order.push_back(s);
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
      return std::lexicographical_compare(T.pool.begin() + T.loff[a], T.pool.begin() + T.loff[a] + T.llen[a], T.pool.begin() + T.loff[b], T.pool.begin() + T.loff[b] + T.llen[b]);
    });
    long long o = 0;
    for (size_t i = 0; i < order.size(); ++i) {
      const size_t s = order[i];
      out_off[i] = o; memcpy(out_tids + o, T.pool.data() + T.loff[s], (size_t)T.llen[s] * 4); out_counts[i] = T.count[s]; o += T.llen[s];
    }
    out_off[order.size()] = o;
    nc = (long long)order.size();
    if ((u64)nc != E.scal[EQC_SC_CLASSES] || (u64)o != E.scal[EQC_SC_POOL]) nc = -4;
  }
  stats[0] = E.growths; stats[1] = (long long)E.scal[EQC_SC_PROBES]; stats[2] = longUnits; stats[3] = E.rounds;
  delete E.tab;
  return nc;
}

}  // extern "C"
