// tests/emu/qm_emu_sanitize.cpp -- TEST-ONLY stand-alone program over the emulation build of the estimation drivers, for a run
// under the host sanitizers: every buffer is a vector of exactly the size the driver's own ensure() asks for, so an index past
// one of them is reported.  Not part of the pytest suite; by hand:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wno-unused \
//       -o qm_emu_sanitize tests/emu/qm_emu_sanitize.cpp && ./qm_emu_sanitize
// The seven-class table of boot_cases.py through quant create / run / fetch, a boot object of 17 replicates over it, and a fold
// of 3000 distinct labels (one of more than EQC_GROUP tids) into a table of 16 slots, which has to grow.
#include <cstdio>
#include "qm_emu_boot.cpp"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

int main() {
  const long long off[] = {0, 1, 3, 4, 6, 7, 10, 13}; const u32 tids[] = {0, 0, 3, 1, 1, 2, 2, 3, 4, 7, 4, 5, 6};
  const u64 cnt[] = {1, 300, 2, 7000, 12, 7686, 5000};
  const long long nT = 9; int err = 0;
  void* q = qe_quant_create(7, off, tids, cnt, nT, nullptr, &err);
  CHECK(q && !err);
  int it = 0; double rel = 0; std::vector<double> alpha((size_t)nT);
  CHECK(!qe_quant_run(q, 50, 10, 1e-2, 1e-8, &it, &rel) && it > 0 && !qe_quant_fetch(q, alpha.data()));
  double sum = 0; for (double a : alpha) sum += a;
  CHECK(sum > 20000.9 && sum < 20001.1 && alpha[8] == 0.0);

  void* b = qe_boot_create(q, 17, 1, &err);
  CHECK(b && !err && qe_quant_destroy(q) == QM_E_STATE);              // (borrowed: refused)
  std::vector<int> its(17); std::vector<double> rels(17), out((size_t)(17 * nT)); std::vector<uint64_t> col(7); long long launches = 0;
  CHECK(qe_boot_run(b, 5, 10, 1e-2, 1e-8, its.data(), rels.data(), &launches) == QM_E_STATE);   // (no counts yet)
  CHECK(!qe_boot_resample(b, 12345, 0) && !qe_boot_run(b, 25, 10, 1e-2, 1e-8, its.data(), rels.data(), &launches) && !qe_boot_fetch(b, out.data()));
  for (int r = 0; r < 17; ++r) {
    uint64_t n = 0;
    CHECK(!qe_boot_fetch_counts(b, r, col.data()));
    for (uint64_t c : col) n += c;
    CHECK(n == 20001);
  }
  CHECK(!qe_boot_set_counts(b, 16, col.data()) && qe_boot_set_counts(b, 17, col.data()) == QM_E_ARG);
  qe_boot_destroy(b);
  CHECK(!qe_quant_destroy(q));

  const long long n = 3000;
  std::vector<long long> loff((size_t)n + 1, 0); std::vector<u32> ltid;
  for (long long i = 0; i < n; ++i) {
    const int len = i == 7 ? 40 : 1 + (int)(i % 3);
    for (int j = 0; j < len; ++j) ltid.push_back((u32)(i * 64 + j));
    loff[(size_t)i + 1] = (long long)ltid.size();
  }
  qm_eqc t; t.longMin = 1;
  CHECK(!eqc_open(&t, 16, 64));
  EqcSrc S{};
  S.tids = (const unsigned char*)ltid.data(); S.stride = 4; S.off = loff.data(); S.n = n;
  CHECK(!eqc_fold(&t, S, loff[(size_t)n], nullptr, t.stream) && !eqc_fold(&t, S, loff[(size_t)n], nullptr, t.stream));
  int64_t nc = 0, nt = 0; uint64_t total = 0;
  CHECK(!eqc_size(&t, &nc, &nt, &total) && nc == n && nt == (int64_t)ltid.size() && total == 2 * (uint64_t)n && t.growths >= 1 && t.longUnits == 2);
  printf("ok: quant %d iterations, boot %lld launches, table grew %lld times over %lld rounds\n", it, launches, (long long)t.growths, (long long)t.rounds);
  return 0;
}
