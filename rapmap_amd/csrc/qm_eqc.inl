// qm_eqc.inl -- equivalence classes on the device: the hit lists of a mapped batch folded into a label -> count table.
//
// A unit's LABEL is the ascending list of the distinct transcript ids of its hit list; the table counts the units (or sums the
// weights) that carried each label.  Written against qm_wave.h: the same source runs lane by lane under -DQM_EMU
// (tests/emu/qm_emu_eqc.cpp).  Every function here is the body of ONE wavefront; qm_eqc_host.inl launches them (qm_exec.h).
//
// Label stage (two launches)
//   eqc_label_groups<8>   eight units per wavefront, eight lanes each: a unit of up to 8 hits is ranked among its group's lanes
//                         (two passes of G cross-lane reads: duplicates, then rank among the first occurrences + key); a longer
//                         unit is put on the long queue (bounded: an entry beyond the capacity is counted, never written -- the host
//                         grows the queue and runs the launch again)
//   eqc_label_queued      one wavefront per queued unit: up to 64 hits the same ranking over the whole wavefront, beyond that an
//                         odd-even transposition sort (in the wave's LDS slab up to EQC_SLAB entries, beyond that in place in the
//                         label buffer), then one pass that drops repeats and sums the key
//   The label of unit u lands at lab[off[u] ..), its length in len[u] (never more than the hit count: the hit offsets serve as
//   label offsets, no capacity of its own), its 64-bit key in key[u].
// Insert stage (rounds of two launches; no wavefront ever waits for another one)
//   eqc_probe_wave        per pending unit: walk the probe sequence of its key over PUBLISHED slots (immutable during the launch),
//                         comparing the full label; equal -> add the weight (equal slots of a wavefront are added up first, one
//                         atomic per slot and wavefront); an unpublished slot -> atomic-min the unit's index into its claim word
//                         and go on the pending queue for the next round
//   eqc_publish_wave      per pending unit: the one whose index the claim word holds copies its label into the bump-allocated pool
//                         and publishes the slot; out of slots or pool -> counted, the claim taken back, nothing written
//   The next round's probe launch finds the slot published and compares.  The host reads the scalars once per round.
#pragma once
#include "qm_wave.h"

namespace qm {

enum { EQC_SC_LONGQ = 0,     // units the group launch put (or would have put) on the long queue
       EQC_SC_PEND = 1,      // entries of the pending queue the probe launch wrote
       EQC_SC_FULL = 2,      // units that probed every slot without finding theirs or a free one
       EQC_SC_TICKETS = 3,   // slot tickets drawn (publish)
       EQC_SC_POOL = 4,      // pool words drawn
       EQC_SC_CLASSES = 5,   // slots published
       EQC_SC_SLOT_OVF = 6, EQC_SC_POOL_OVF = 7,
       EQC_SC_PROBES = 8,    // published slots that held another label (true collisions and neighbours)
       EQC_SC_SUM = 9,       // qm_eqc_sum_kernel's result
       EQC_SC_WORDS = 16 };
#define EQC_SLAB 2048        // entries of a wavefront's LDS slab (long units)
#define EQC_GROUP 8          // lanes per unit in the group launch

struct EqcSrc {              // the units of a fold and where their labels go
  const unsigned char* tids; int stride;   // hit j's tid: *(const u32*)(tids + j * stride) (32: qm_hit records, 4: plain lists)
  const long long* off;      // [n + 1]
  long long n;
  u32* lab; u32* len; u64* key;
  long long* longq; u64 longCap;
  u64* scal; u64 keyMask;
};
struct EqcSet {              // labelled units as the insert stage reads them (a fold's, or an old table's slots when it grows)
  const u32* lab; const long long* off; const u32* len; const u64* key; const u64* w; long long n;
};
struct EqcTable {
  u64* key;                  // 0: not published
  u64* claim;                // smallest unit index that wants the unpublished slot (~0: nobody)
  long long* loff; u32* llen; u64* count; u32* pool;
  u64 mask, maxClasses, poolCap;
  u64* scal;
};

QM_DEV u64 eqc_mix(u64 x) {
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ULL; x ^= x >> 27; x *= 0x94d049bb133111ebULL; x ^= x >> 31;
  return x;
}
QM_DEV u64 eqc_tid_hash(u32 t) { return eqc_mix((u64)t + 0x9e3779b97f4a7c15ULL); }
// the key of a label from the sum of its tids' hashes (order-free: summed in whatever order the lanes hold them); never 0
QM_DEV u64 eqc_key(u64 hsum, u32 n, u64 keyMask) { return (eqc_mix(hsum ^ ((u64)n << 32)) & keyMask) | (1ULL << 63); }
QM_DEV u32 eqc_load_tid(const EqcSrc& S, long long j) { return *(const u32*)(S.tids + j * (long long)S.stride); }

// `push` lanes append unit[l] to the long queue: one atomic per wavefront; entries beyond the capacity are counted only
QM_DEV void eqc_push_long(const EqcSrc& S, const LV<long long>& unit, const LV<bool>& push) {
  const u64 pm = ballot(push);
  if (!pm) return;
  const int lead = ctz64(pm);
  LV<u64> b;
  QM_LANES(l) { b[l] = 0; if (l == lead) b[l] = atomic_add_u64(&S.scal[EQC_SC_LONGQ], (u64)popc64(pm)); }
  const u64 b0 = read_lane(b, lead);
  QM_LANES(l) if (push[l]) { const u64 pos = b0 + (u64)popc64(pm & lanemask_lt(l)); if (pos < S.longCap) S.longq[pos] = unit[l]; }
}

// Groups of G lanes (8 or 64), one unit each (unit[l]: the unit of lane l's group, -1: none).  A unit of up to G hits is labelled;
// a longer one is left alone (over[l] tells the caller).
template <int G>
QM_DEV void eqc_label_groups(const EqcSrc& S, const LV<long long>& unit, LV<bool>& over) {
  LV<u32> v, vi; LV<bool> valid, dup; LV<int> cnt, idx, rank; LV<u64> hs;
  QM_LANES(l) {
    const long long u = unit[l]; const int j = l & (G - 1);
    long long o = 0, c = 0;
    if (u >= 0) { o = S.off[u]; c = S.off[u + 1] - o; }
    over[l] = c > G; valid[l] = c <= G && j < c; cnt[l] = c <= G ? (int)c : 0;
    v[l] = valid[l] ? eqc_load_tid(S, o + j) : 0u;
    dup[l] = false; rank[l] = 0; hs[l] = 0;
  }
  const u64 vm = ballot(valid);
  const int lim = wave_max(cnt);                               // no group of this wavefront holds more
  for (int i = 1; i < lim; ++i) {                              // pass 1: a lane is a repeat when a lower lane of its group holds its tid
    QM_LANES(l) idx[l] = (l & ~(G - 1)) + ((l - i) & (G - 1));  // ... the lane i below, wrapping: only the ones really below count
    wave_read(v, idx, vi);
    QM_LANES(l) if (valid[l] && idx[l] < l && ((vm >> idx[l]) & 1) && vi[l] == v[l]) dup[l] = true;
  }
  const u64 fm = vm & ~ballot(dup);                            // first occurrences
  for (int i = 0; i < lim; ++i) {                              // pass 2: rank among the first occurrences, sum of their hashes
    QM_LANES(l) idx[l] = (l & ~(G - 1)) + i;
    wave_read(v, idx, vi);
    QM_LANES(l) if ((fm >> idx[l]) & 1) { hs[l] += eqc_tid_hash(vi[l]); if (vi[l] < v[l]) rank[l]++; }
  }
  QM_LANES(l) {
    const long long u = unit[l];
    if (u < 0 || over[l]) continue;
    if (valid[l] && !dup[l]) S.lab[S.off[u] + rank[l]] = v[l];
    if ((l & (G - 1)) == 0) {
      const int gb = l & ~(G - 1);
      const u32 n = (u32)popc64(G == 64 ? fm : ((fm >> gb) & ((1ULL << (G & 63)) - 1)));
      S.len[u] = n; S.key[u] = n ? eqc_key(hs[l], n, S.keyMask) : 0;
    }
  }
}

// the group launch: wavefront `wave` labels units [wave * 64 / G, ...) and queues the long ones
QM_DEV void eqc_label_wave(const EqcSrc& S, long long wave) {
  LV<long long> unit; LV<bool> over, push;
  QM_LANES(l) { const long long u = wave * (64 / EQC_GROUP) + l / EQC_GROUP; unit[l] = u < S.n ? u : -1; }
  eqc_label_groups<EQC_GROUP>(S, unit, over);
  QM_LANES(l) push[l] = over[l] && (l & (EQC_GROUP - 1)) == 0;
  eqc_push_long(S, unit, push);
}

// a unit of more than 64 hits: sort (odd-even transposition, any length, in place), drop repeats, sum the key.  BufT: the wave's LDS
// slab (an LDS pointer: DS instructions, never FLAT ones -- a generic pointer that may land in LDS makes every access a FLAT one, and
// the two neighbours a lane loads become one 8-byte access that LDS only takes at an 8-byte boundary) or the label buffer itself
template <typename BufT>
QM_DEV void eqc_sort_unique(const EqcSrc& S, long long u, long long o, long long c, BufT buf) {
  QM_LANES(l) for (long long i = l; i < c; i += 64) buf[i] = eqc_load_tid(S, o + i);
  wave_fence();
  int quiet = 0;                                               // two phases in a row without a swap: sorted
  for (long long ph = 0; ph < c && quiet < 2; ++ph) {
    LV<bool> sw;
    QM_LANES(l) {
      bool s = false;
      for (long long i = (ph & 1) + 2 * l; i + 1 < c; i += 128) {
        const u32 a = buf[i], b = buf[i + 1];
        if (a > b) { buf[i] = b; buf[i + 1] = a; s = true; }
      }
      sw[l] = s;
    }
    wave_fence();
    quiet = ballot(sw) ? 0 : quiet + 1;
  }
  long long wpos = 0;                                          // (never ahead of the read position: in place is safe)
  LV<u64> hs; QM_LANES(l) hs[l] = 0;
  for (long long b = 0; b < c; b += 64) {
    LV<u32> x; LV<bool> keep;
    QM_LANES(l) { const long long i = b + l; keep[l] = false; x[l] = 0; if (i < c) { x[l] = buf[i]; keep[l] = i == 0 || buf[i - 1] != x[l]; } }
    wave_fence();
    const u64 km = ballot(keep);
    QM_LANES(l) if (keep[l]) { S.lab[o + wpos + popc64(km & lanemask_lt(l))] = x[l]; hs[l] += eqc_tid_hash(x[l]); }
    wave_fence();
    wpos += popc64(km);
  }
  u64 tot = 0;
  for (int i = 0; i < 64; ++i) tot += read_lane(hs, i);
  QM_LANES(l) if (l == 0) { S.len[u] = (u32)wpos; S.key[u] = eqc_key(tot, (u32)wpos, S.keyMask); }
}

QM_DEV void eqc_label_long(const EqcSrc& S, long long u, QM_LDS(u32)* slab) {
  const long long o = S.off[u], c = S.off[u + 1] - o;
  if (c <= EQC_SLAB) eqc_sort_unique(S, u, o, c, slab);
  else eqc_sort_unique(S, u, o, c, S.lab + o);
}

// the queue launch: wavefront `wave` labels queue entry `wave`
QM_DEV void eqc_label_queued(const EqcSrc& S, long long wave, QM_LDS(u32)* slab) {
  const long long u = S.longq[wave];
  const long long c = S.off[u + 1] - S.off[u];
  if (c <= 64) { LV<long long> unit; LV<bool> over; QM_LANES(l) unit[l] = u; eqc_label_groups<64>(S, unit, over); }
  else eqc_label_long(S, u, slab);
}

// ---- insert stage.  A queue entry: probe << 32 | unit.
QM_DEV void eqc_probe_wave(const EqcTable& T, const EqcSet& S, const u64* qin, long long nin, u64* qout, long long wave, int aggregate) {
  LV<bool> add, pend; LV<u64> slot, wv, ent; LV<int> np;
  QM_LANES(l) {
    add[l] = false; pend[l] = false; slot[l] = 0; wv[l] = 0; ent[l] = 0; np[l] = 0;
    const long long i = wave * 64 + l;
    if (i >= nin) continue;
    const u64 e = qin ? qin[i] : (u64)i;
    const u32 u = (u32)e; u64 p = e >> 32;
    const u32 n = S.len[u];
    if (!n) continue;                                          // no hits: contributes nothing
    const u64 k = S.key[u]; const u32* L = S.lab + S.off[u];
    const u64 h = eqc_mix(k);
    for (;; ++p) {
      if (p > T.mask) { pend[l] = true; atomic_add_u64(&T.scal[EQC_SC_FULL], 1); break; }   // every slot seen: the host grows the table
      const u64 s = (h + p) & T.mask;
      const u64 kk = T.key[s];
      if (!kk) {                                               // not published: ask for it (the claim only ever falls: a stale read costs an atomic, no more)
        if (T.claim[s] > (u64)u) atomic_min_u64(&T.claim[s], (u64)u);
        pend[l] = true; break;
      }
      if (kk == k && T.llen[s] == n) {
        const u32* P = T.pool + T.loff[s];
        u32 j = 0; while (j < n && P[j] == L[j]) ++j;
        if (j == n) { add[l] = true; slot[l] = s; wv[l] = S.w ? S.w[u] : 1; break; }
      }
      np[l]++;
    }
    ent[l] = (p << 32) | u;
  }
  const u64 pm = ballot(pend);
  if (pm) {                                                    // one queue cursor bump per wavefront
    const int lead = ctz64(pm);
    LV<u64> b;
    QM_LANES(l) { b[l] = 0; if (l == lead) b[l] = atomic_add_u64(&T.scal[EQC_SC_PEND], (u64)popc64(pm)); }
    const u64 b0 = read_lane(b, lead);
    QM_LANES(l) if (pend[l]) qout[b0 + (u64)popc64(pm & lanemask_lt(l))] = ent[l];   // (the queue holds as many entries as the launch has units)
  }
  lane_scan_add(np);                                           // a statistic: summed over the wavefront, one atomic
  const int nprobes = read_lane(np, 63);
  if (nprobes) { QM_LANES(l) if (l == 0) atomic_add_u64(&T.scal[EQC_SC_PROBES], (u64)nprobes); }
  u64 am = ballot(add);
  if (!aggregate) { QM_LANES(l) if (add[l]) atomic_add_u64(&T.count[slot[l]], wv[l]); return; }
  while (am) {                                                 // class sizes are skewed: the lanes of one slot add up first
    const int lead = ctz64(am);
    const u64 s = read_lane(slot, lead);
    LV<bool> same;
    QM_LANES(l) same[l] = add[l] && slot[l] == s;
    const u64 sm = ballot(same);
    u64 tot = 0;
    if (!S.w) tot = (u64)popc64(sm);
    else for (u64 mm = sm; mm; mm &= mm - 1) tot += read_lane(wv, ctz64(mm));
    QM_LANES(l) if (l == lead) atomic_add_u64(&T.count[s], tot);
    am &= ~sm;
  }
}

QM_DEV void eqc_publish_wave(const EqcTable& T, const EqcSet& S, const u64* q, long long nq, long long wave) {
  QM_LANES(l) {
    const long long i = wave * 64 + l;
    if (i >= nq) continue;
    const u64 e = q[i]; const u32 u = (u32)e; const u64 p = e >> 32;
    if (p > T.mask) continue;
    const u64 k = S.key[u];
    const u64 s = (eqc_mix(k) + p) & T.mask;
    if (T.key[s] || T.claim[s] != (u64)u) continue;            // published already (cannot be: pending), or another unit won
    const u32 n = S.len[u];
    if (atomic_add_u64(&T.scal[EQC_SC_TICKETS], 1) >= T.maxClasses) { atomic_add_u64(&T.scal[EQC_SC_SLOT_OVF], 1); T.claim[s] = ~0ULL; continue; }
    const u64 o = atomic_add_u64(&T.scal[EQC_SC_POOL], (u64)n);
    if (o + n > T.poolCap) { atomic_add_u64(&T.scal[EQC_SC_POOL_OVF], 1); T.claim[s] = ~0ULL; continue; }
    const u32* L = S.lab + S.off[u];
    for (u32 j = 0; j < n; ++j) T.pool[o + j] = L[j];
    T.loff[s] = (long long)o; T.llen[s] = n; T.count[s] = 0; T.key[s] = k;
    atomic_add_u64(&T.scal[EQC_SC_CLASSES], 1);
  }
}

}  // namespace qm
