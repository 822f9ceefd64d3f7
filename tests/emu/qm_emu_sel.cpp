// tests/emu/qm_emu_sel.cpp -- TEST-ONLY lane emulation of the -s question scorer and the strip alignments by themselves: sel_side_score<1> with
// SelRedOne and sel_tasks_strip of rapmap_amd/csrc/qm_sel.inl compiled with -DQM_EMU.  The entry point builds a PairBatch / SelBatch from flat
// arrays -- one unit and one hit per question, the reads back to back in one buffer as the product keeps them --, scores every question as
// qm_sel_score_kernel does with one lane per question, and then runs the strip alignments over the questions with kind & 4, four at a time,
// as qm_sel_strip_kernel does.  (tests/device/qm_probe.hip: qp_sel_side / qp_sel_strip are the same on the device.)
#define QM_EMU
#include "../../rapmap_amd/csrc/qm_mapper.inl"

#include <string.h>
#include <vector>

using namespace qm;

extern "C" {

int qe_sel_max_read_len(void) { return QM_MAX_READ_LEN; }

// nq questions.  reads[roffs[nq]]: question x asks about reads[roffs[x] .. roffs[x + 1]); text[ntext] with ntx transcripts txp_off / txp_len;
// qd: nq x {tid, pos, fwd, chain status, multi-mapping unit}; prm: {policy, match, mismatch, gap open, gap extend, band, run the strip pass}.
// Out, per question: kind, tsc (0x5A5A5A5A: never written), key, task[9] = {written, read offset, target offset, gslot, rl, roff, rlen,
// tlen1, fwd} (written 0: tasks[x] still holds the 0xEE the caller's record was filled with; the other eight are 0 then).
// Returns the number of strip alignments run, -1 for a bad argument.
int qe_sel_side(int nq, const unsigned char* reads, const long long* roffs, const unsigned char* text, long long ntext, int ntx, const u32* txp_off,
                const int* txp_len, const int* qd, const int* prm, int* kind, int* tsc, u64* key, long long* task) {
  if (nq < 1 || ntx < 1 || roffs[0] < 0) return -1;
  for (int t = 0; t < ntx; ++t) if (txp_len[t] < 0 || (long long)txp_off[t] + txp_len[t] > ntext) return -1;
  for (int x = 0; x < nq; ++x) {
    const int* d = qd + 5 * x;
    if (roffs[x + 1] < roffs[x] || d[0] < 0 || d[0] >= ntx || d[1] < -(1 << 24) || d[1] > (1 << 24)) return -1;
  }
  const size_t n = (size_t)nq;
  std::vector<u32> cnt(n + 1, 0);
  std::vector<qm_hit> tmp(n);
  std::vector<SelSide> sides(n);
  std::vector<SelTask> tasks(n);
  std::vector<int> tscv(2 * n, 0x5A5A5A5A), tref(2 * n, 0x5A5A5A5A);
  std::vector<u64> torder2(n + 4, 0);
  memset(tasks.data(), 0xEE, sizeof(SelTask) * n);
  memset(sides.data(), 0xEE, sizeof(SelSide) * n);
  for (size_t x = 0; x < n; ++x) {
    const int* d = qd + 5 * x;
    qm_hit h; memset(&h, 0, sizeof(h));
    h.tid = (u32)d[0]; h.pos = d[1]; h.fwd = d[2] ? 1 : 0; h.mate_is_fwd = 1; h.read_len = (u32)(roffs[x + 1] - roffs[x]); h.aln_score = d[3];
    tmp[x] = h;
    cnt[x] = d[4] ? 2u : 1u;
    sides[x].u = (long long)x; sides[x].g = 2 * (long long)x; sides[x].nth = 0;
  }
  u64 nsides = (u64)n, ntasks2 = 0;
  PairBatch P; memset(&P, 0, sizeof(P));
  P.n = nq; P.paired = 0; P.off1 = roffs; P.off2 = roffs; P.cnt = cnt.data(); P.max_num_hits = 200;
  SelBatch A; memset(&A, 0, sizeof(A));
  A.seq1 = reads; A.seq2 = reads; A.text = text; A.txp_off = txp_off; A.txp_len = txp_len; A.tmp = tmp.data();
  A.tsc = tscv.data(); A.tref = tref.data(); A.sides = sides.data(); A.nsides = &nsides; A.tasks = tasks.data();
  A.torder2 = torder2.data(); A.ntasks2 = &ntasks2; A.u0 = 0; A.u1 = nq;
  A.policy = prm[0]; A.match = prm[1]; A.mismatch = prm[2]; A.gap_open = prm[3]; A.gap_extend = prm[4]; A.bandwidth = prm[5];
  A.min_score_fraction = 0.65;
  for (u64 x = 0; x < nsides; ++x) sel_side_score<1>(P, A, (long long)x, 0, SelRedOne());
  for (size_t x = 0; x < n; ++x) if (sides[x].kind & 4) torder2[ntasks2++] = (u64)x;
  if (prm[6]) { static StripMem SM; for (u64 t = 0; t < ntasks2; t += 4) sel_tasks_strip(A, t, ntasks2, SM); }
  std::vector<unsigned char> fill(sizeof(SelTask), 0xEE);
  for (size_t x = 0; x < n; ++x) {
    kind[x] = sides[x].kind; key[x] = sides[x].key; tsc[x] = tscv[2 * x];
    long long* o = task + 9 * x;
    for (int i = 0; i < 9; ++i) o[i] = 0;
    if (memcmp(&tasks[x], fill.data(), sizeof(SelTask)) == 0) continue;
    const SelTask& t = tasks[x];
    o[0] = 1; o[1] = (long long)(t.rd - reads); o[2] = (long long)(t.tx - text); o[3] = t.gslot; o[4] = t.rl; o[5] = t.roff; o[6] = t.rlen; o[7] = t.tlen1; o[8] = t.fwd;
  }
  return (int)ntasks2;
}

}  // extern "C"
