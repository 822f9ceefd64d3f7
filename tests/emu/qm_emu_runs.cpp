// tests/emu/qm_emu_runs.cpp -- TEST-ONLY: a paired batch through ONE headline kernel's wave driver (duo_wave or lean_wave) under a chosen
// schedule -- nw waves that take runs of `run` neighbouring pairs (rapmap_amd/csrc/qm_grid.h) -- and on to hit records the way the
// library goes on behind that kernel (qm_host.hip, run_stage_a / run_stage_b): the reads the kernel marked are queued and mapped by the
// general kernel, stage B merges what was not merged in the wavefront, the pair kernel's own counters are added to stage B's.
// tests/test_wave_runs_emu.py holds the result to the oracle.  Built on the emulation's own unit (its includes, slabs and read passes).
#include "qm_emu.cpp"

extern "C" {

// kernel: 0 the pair kernel (pairs merged in the wavefront), 1 qm_lean_kernel's paired edition.  Dense index, default-shaped options
// (no -s).  out_stats: reads the kernel left, pairs it merged, status bits of all passes (| 0x100: the general kernel set a read aside,
// 8: the kernel's own count of them differs).
int qe_runs_map(int k, const unsigned char* text, long long n, const u32* SA, long long nSA, const void* sainfo, const void* slots,
                unsigned long long hmask, const qm_opts* o, long long nunits, const unsigned char* seq1, const long long* off1,
                const unsigned char* seq2, const long long* off2, int kernel, int nw, int run, long long* hit_offsets, qm_hit** hits_out,
                unsigned long long* counters, long long* out_stats) {
  if (nw < 1 || !(run == 1 || run == 2 || run == 4 || run == 8) || !seq2 || o->sel_aln) return 1;
  const int rs = run == 8 ? 3 : run == 4 ? 2 : run == 2 ? 1 : 0;
  DevIndex ix; memset(&ix, 0, sizeof(ix));
  ix.text = text; ix.n = n; ix.SA = SA; ix.nSA = nSA; ix.sainfo = (const SaInfo*)sainfo; ix.slots = (const Bucket*)slots; ix.hmask = hmask; ix.k = k;
  std::vector<SaExt> saext((size_t)nSA);                    // the replica's SaExt table (build_saext_kernel)
  for (long long i = 0; i < nSA; ++i) { const SaInfo si = ((const SaInfo*)sainfo)[i]; saext[(size_t)i] = saext_entry(text, n, (long long)SA[i] + k, si.tid, si.pos); }
  ix.saext = saext.data();
  const long long nreads = 2 * nunits;
  std::vector<u32> lcnt(nreads + 1, 0), pcnt(nunits + 1, 0); std::vector<long long> loff(nreads + 1, 0);
  std::vector<u64> lists, gs(QM_GSCR_U64);
  u64 scal[QM_SC_WORDS]; int status = 0;
  ReadBatch B; memset(&B, 0, sizeof(B));
  B.seq1 = seq1; B.off1 = off1; B.seq2 = seq2; B.off2 = off2; B.nreads = nreads;
  B.lcnt = lcnt.data(); B.loff = loff.data(); B.cursor = scal; B.status = &status; B.gscratch = gs.data();
  B.strict_check = o->strict_check; B.max_interval = o->max_interval; B.quasi_cov = o->quasi_cov; B.sensitive = o->sensitive; B.fuzzy = o->fuzzy;
  B.max_mmp_ext = o->max_mmp_extension > 0 ? o->max_mmp_extension : 7;
  if (kernel == 0 && !o->fuzzy) { B.pair_cnt = pcnt.data(); B.max_num_hits = o->max_num_hits; B.no_orphans = o->no_orphans; B.no_dovetail = o->no_dovetail; }
  long long cap = nreads * 8 + ((long long)nw + 16) * QM_CHUNK, left = 0;
  int slow = 0;
  while (true) {
    lists.assign((size_t)cap, 0);
    B.lists = lists.data(); B.lists_cap = cap; memset(scal, 0, sizeof(scal)); status = 0;
    std::fill(lcnt.begin(), lcnt.end(), 0u); std::fill(pcnt.begin(), pcnt.end(), 0u);
    // the first launch: the headline kernel's waves, each on a slab that holds whatever it held
    if (kernel == 0) duo_dispatch(false, B.quasi_cov > 0.0, [&](auto H, auto C) {
      for (int w = 0; w < nw; ++w) duo_wave<decltype(H)::value, decltype(C)::value>(ix, B, w, nw, garbage_slab<DuoMem>(), rs);
    });
    else lean_dispatch(true, false, false, [&](auto P, auto S, auto H) {
      for (int w = 0; w < nw; ++w) lean_wave<decltype(P)::value, decltype(S)::value, decltype(H)::value, false, false>(ix, B, w, nw, garbage_slab<LeanMem>(), rs);
    });
    // what it marked, gathered (gather_queue) and mapped by the general kernel where the first launch would have put it (pass_lean_leftovers)
    std::vector<long long> q;
    for (long long r = 0; r < nreads; ++r) if (lcnt[r] == QM_LCNT_LEAN) q.push_back(r);
    left = (long long)q.size();
    if ((long long)scal[QM_SC_LEANQ] != left) status |= 8;
    if (!q.empty() && !(status & 1)) {
      ReadBatch Q = B; Q.slowq = q.data(); Q.nreads = left;
      emu_read(2, B.sensitive ? 0 : QM_F_NIP, ReadPass{ix, Q, gs.data(), nullptr, nullptr, false, nullptr});
    }
    slow = scal[QM_SC_SLOWCNT] > 0 ? 0x100 : 0;
    if (!(status & 1)) break;
    cap *= 4;
  }
  // stage B: count, scan, write; a pair merged in the wavefront has its count already and adds nothing to the counters here
  PairBatch P; memset(&P, 0, sizeof(P));
  std::vector<u32> hc(nunits + 1, 0);
  long long merged = 0;
  for (long long u = 0; u < nunits; ++u) if (lcnt[2 * u] == QM_LCNT_PAIR) { hc[u] = pcnt[u]; ++merged; }
  P.n = nunits; P.paired = 1; P.off1 = off1; P.off2 = off2; P.lcnt = lcnt.data(); P.loff = loff.data(); P.lists = lists.data(); P.cnt = hc.data();
  P.max_num_hits = o->max_num_hits; P.no_orphans = o->no_orphans; P.no_dovetail = o->no_dovetail; P.fuzzy = o->fuzzy;
  UnitCounters uc = {0, 0, 0, 0, 0, 0};
  for (long long u = 0; u < nunits; ++u) hc[u] = (u32)unit_merge(P, u, nullptr, 0, &uc);
  hit_offsets[0] = 0;
  for (long long u = 0; u < nunits; ++u) hit_offsets[u + 1] = hit_offsets[u] + hc[u];
  qm_hit* out = (qm_hit*)malloc(sizeof(qm_hit) * (size_t)(hit_offsets[nunits] + 1));
  for (long long u = 0; u < nunits; ++u) if (hc[u]) unit_merge(P, u, out + hit_offsets[u], (int)hc[u], nullptr);
  *hits_out = out;
  counters[0] = uc.pe + scal[1]; counters[1] = uc.se + scal[2]; counters[2] = uc.tot + scal[3]; counters[3] = uc.reads + scal[4];
  counters[4] = uc.tooMany + scal[5]; counters[5] = uc.mapped + scal[6];
  out_stats[0] = left; out_stats[1] = merged;
  out_stats[2] = status | slow;
  return 0;
}

}  // extern "C"
