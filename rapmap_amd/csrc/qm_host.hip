// qm_host.hip -- host side of libqmap_mi355.so: q5 index reader (mmap), HBM replica,
// and the C ABI declared in include/qmap_mi355.h.
//
// Reader follows the writers in src/RapMapSAIndexer.cpp:109-110,242-243 (sa.bin),
// :694-731 (rsd.bin, txpInfo.bin), :433-441 + include/sparsepp/spp.h:2355-2366 (hash.bin),
// include/IndexHeader.hpp:45-57 (header.json); semantics of
// RapMapSAIndex::load (src/RapMapSAIndex.cpp:97-176).  Files are mmap'd, never
// deserialised into containers; the GPU flattens them (qm_kernels.hip).
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>
#include <thread>
#include <map>
#include <memory>
#include <mutex>
#include <condition_variable>
#include <functional>

#include "qm_mapper.inl"
#include "qm_lean.inl"
#include "qm_device.h"
#include "qm_phflat.h"

using namespace qm;

static thread_local char g_err[512] = "";
static int fail(int code, const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
  return code;
}
#define HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) return fail(QM_E_NOGPU, "%s: %s", #x, hipGetErrorString(_e)); } while (0)

struct MMap {
  void* p = nullptr; size_t len = 0;
  int open(const std::string& path) {
    int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) return -1;
    struct stat st; if (fstat(fd, &st) != 0) { ::close(fd); return -1; }
    len = (size_t)st.st_size;
    if (len == 0) { ::close(fd); return -1; }
    p = mmap(nullptr, len, PROT_READ, MAP_PRIVATE, fd, 0);
    ::close(fd);
    if (p == MAP_FAILED) { p = nullptr; return -1; }
    return 0;
  }
  void close() { if (p) munmap(p, len); p = nullptr; }
};

struct qm_index {
  std::string dir;
  int k = 31; bool big = false, perfect = false;
  MMap sa, txp, rsd, hash;
  // SA entries, transcript offsets and interval bounds are UNSIGNED 32-bit from here on (qm_mapper.inl, struct Iv).  A BigSA index
  // (int64 on disk: text > 2^31 - 1 characters, src/RapMapSAIndexer.cpp:682-683) is narrowed into the *Narrow vectors at open.
  const uint32_t* SA = nullptr; int64_t nSA = 0;
  std::vector<std::string> names;
  const uint32_t* offsets = nullptr; int64_t nTxp = 0;
  std::vector<uint32_t> saNarrow, offNarrow, phDataNarrow; std::vector<uint8_t> hashNarrow;
  const uint8_t* text = nullptr; int64_t n = 0;
  const uint32_t* completeLens = nullptr;
  std::vector<int64_t> lens;
  const uint8_t* hashRecs = nullptr; int64_t nKeys = 0;   // K x 16 B records
  uint64_t rsdBits = 0;
  // perfect-hash flavour (hash_info.bph / hash_info.val)
  MMap bph, val;
  struct PhLevel { uint64_t domain, nchar, nranks; const uint8_t* words; const uint8_t* ranks; };
  std::vector<PhLevel> phLevels;
  uint64_t phLastRank = 0, phNelem = 0;
  std::vector<std::pair<uint64_t, uint64_t>> phFinal;
  const uint8_t* phData = nullptr; const uint8_t* phLens = nullptr;
  std::vector<std::pair<uint32_t, uint32_t>> phOverflow;
};

// A device array that owns its memory: the pointer, the capacity in elements, freed with its owner.  Every device buffer of the
// replica, the context and the estimation objects (the equivalence-class table's six arrays included) is one of these (arrays of other types' records: bytes, cast where read).
template <typename T>
struct DevBuf {
  T* p = nullptr; int64_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  operator T*() const { return p; }
  void release() { if (p) hipFree(p); p = nullptr; cap = 0; }
  void swap(DevBuf& o) { std::swap(p, o.p); std::swap(cap, o.cap); }
  // room for `want` elements (contents are not kept)
  int ensure(int64_t want, int64_t minGrow = 0) {
    if (want <= cap && p) return QM_OK;
    if (p) hipFree(p);
    p = nullptr;
    int64_t nc = want + minGrow;
    if (cap > 0 && nc < cap + cap / 2) nc = cap + cap / 2;     // a buffer that grows again grows by half: callers whose batches vary in size (the
                                                               // compat header's batching service) stop paying a round of hipFree / hipMalloc per new maximum
    if (nc > want + minGrow && hipMalloc((void**)&p, (size_t)nc * sizeof(T)) != hipSuccess) { p = nullptr; (void)hipGetLastError(); nc = want + minGrow; }   // no room for the slack: the exact size
    if (!p && hipMalloc((void**)&p, (size_t)nc * sizeof(T)) != hipSuccess) { cap = 0; return fail(QM_E_NOMEM, "hipMalloc of %lld bytes failed", (long long)(nc * sizeof(T))); }
    cap = nc;
    return QM_OK;
  }
};
// ... and its sibling in pinned host memory, of a fixed size: allocated at first use
template <typename T>
struct PinBuf {
  T* p = nullptr;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() { if (p) hipHostFree(p); }
  operator T*() const { return p; }
  int ensure(size_t n) {
    if (!p) HIPCHK(hipHostMalloc((void**)&p, n * sizeof(T), hipHostMallocDefault));
    return QM_OK;
  }
};

// The index replica of one device: built by the first context on (index, device) (build_replica), shared read-only by every later
// one (one context per host thread is the intended use: a Salmon-style caller has many), freed with the last of them.
struct Replica {
  int device = 0;
  DevBuf<uint8_t> text; DevBuf<uint32_t> SA; DevBuf<unsigned char> sainfo, slots; uint64_t cap = 0;   // (SaInfo / Bucket records; cap: buckets)
  const PhIndex* ph = nullptr; PhIndex hPh; std::deque<DevBuf<unsigned char>> phAllocs;   // the compact -p image: PhIndex on the device (in phAllocs, like its arrays), its host copy
  DevBuf<uint32_t> txpOff; DevBuf<int32_t> txpLen; int64_t devBytes = 0;
  std::mutex sanextMu; DevBuf<unsigned int> sanext;        // -s: built by the first -s call of any context of this replica
  DevBuf<unsigned char> saext;                              // the packed characters behind every suffix's k-mer (SaExt), or empty
  DevBuf<unsigned char> saext2; bool saext2Tried = false;   // ... the wide edition (SaExt2), built when reads of 129 .. 256 characters first ask (sanextMu)
  DevBuf<u64> gcMask; DevBuf<uint32_t> gcRank; bool gcBuilt = false;   // the GC rank structure over the text, built by the first qm_gcb (sanextMu; qm_gcb_host.inl)
  ~Replica() { hipSetDevice(device); }                      // (then the members free themselves)
};
static std::mutex g_repMu;
static std::map<std::pair<const qm_index*, int>, std::weak_ptr<Replica>> g_reps;   // key: index, device * 2 + (compact perfect hash)
static std::map<std::pair<const qm_index*, int>, std::shared_ptr<std::mutex>> g_repBuild;   // one builder per key at a time

// What the last call on a context reported about itself: everything qm_ctx_stat and qm_fetch_skipped read.  The default state is a
// call that used none of the kernels; the stages fill in what they run.
struct CallStats {
  int64_t relaunches = 0, slowReads = 0;
  int64_t leanReads = -1, leanDeferred = 0;       // leanReads: reads the lean kernel was launched over (-1: not used)
  int64_t selQuestions = 0, kswTasks = 0, stripTasks = 0;   // -s: alignment questions beyond PERFECT chains, ksw2 / strip alignments run for them
  int64_t defer[4] = {0, 0, 0, 0};                // QM_STAT_DEFER_*
  int64_t nPass = 0;                              // QM_STAT_N_PASS_READS: reads the N-aware pass of stage A mapped
  int64_t duoPairs = -1, duoMerged = 0;           // pairs the pair kernel was launched over (-1: not used), pairs it merged itself
  int64_t skipped = 0; std::vector<uint64_t> skipList;   // reads skipped, not mapped (ReadBatch::skiplist): how many, the first QM_SKIP_CAP of them
  // A call mapped in parts (map_device_split) reports its parts' sums.  The kernels' own figures count only where a part ran that
  // kernel: the lean reads stay -1 until a part ran a lean kernel, the merged pairs are those of the parts that ran the pair kernel,
  // and the pair kernel's pair count stays -1 (an unsplit call only: qmap_mi355.h).  firstRead: the part's read 0 in the whole batch.
  void add_part(const CallStats& p, int64_t firstRead) {
    relaunches += p.relaunches; slowReads += p.slowReads; nPass += p.nPass;
    selQuestions += p.selQuestions; kswTasks += p.kswTasks; stripTasks += p.stripTasks;
    for (int t = 0; t < 4; ++t) defer[t] += p.defer[t];
    if (p.leanReads >= 0) { leanReads = (leanReads < 0 ? 0 : leanReads) + p.leanReads; leanDeferred += p.leanDeferred; }
    if (p.duoPairs >= 0) duoMerged += p.duoMerged;
    skipped += p.skipped;
    const uint64_t idx = (1ULL << 56) - 1;        // (an entry: the read below, the reason above)
    for (uint64_t e : p.skipList)
      if (skipList.size() < QM_SKIP_CAP) skipList.push_back(((e & idx) + (uint64_t)firstRead) | (e & ~idx));
  }
};
// ... and what it left to fetch: the result's size and times, and which per-read outputs the buffers hold (-1: none)
struct LastResult {
  int64_t units = -1, hits = 0; bool paired = false;
  double mapMs = 0, totalMs = 0;
  int64_t ivReads = -1, ivTotal = 0, foundReads = -1, listReads = -1, listWords = 0, tooManyUnits = -1;
  int64_t stReads = -1, stUnits = -1;             // qm_fetch_stages
  void invalidate() { *this = LastResult(); }
};
static qm_counters counters_from(const u64* hscal) { return qm_counters{hscal[1], hscal[2], hscal[3], hscal[4], hscal[5], hscal[6]}; }
static qm_counters& operator+=(qm_counters& a, const qm_counters& b) {
  a.pe_hits += b.pe_hits; a.se_hits += b.se_hits; a.tot_hits += b.tot_hits; a.num_reads += b.num_reads; a.too_many_hits += b.too_many_hits; a.mapped += b.mapped;
  return a;
}

struct qm_ctx {
  const qm_index* ix = nullptr;
  std::shared_ptr<Replica> rep;
  int device = 0, numCU = 256;
  hipStream_t stream = nullptr, copyStream = nullptr;      // kernels / host-buffer uploads (overlapped chunk by chunk)
  // the replica's two tables that are built lazily and its size, as this context last saw them under the replica's sanextMu
  // (ensure_sanext, ensure_saext2): another context's first -s call may be writing the replica's own fields
  unsigned int* d_sanext = nullptr;                         // -s: text characters behind every suffix's k-mer
  void* d_saext2 = nullptr;                                 // the wide edition of the replica's SaExt table, once built
  int64_t devBytes = 0;
  hipStream_t planStream = nullptr;                         // -s: the plan kernels of the later chunks, under the ksw2 kernel of the earlier ones
  hipEvent_t evPlan[QM_SEL_CHUNKS_B + 1] = {};              // ... [i]: chunk i planned; [last]: the plan stream may start
  DevBuf<u64> d_ntk;                                        // ... per chunk: a task counter, then (at QM_SEL_CHUNKS_B + i) a counter of alignment questions
  hipEvent_t ev0 = nullptr, ev1 = nullptr, evA = nullptr, evB = nullptr, evCopy = nullptr, evStage[2] = {nullptr, nullptr};
  hipEvent_t evP0 = nullptr, evP1 = nullptr;                // around the second launches of stage A (the N-aware pass, the general kernel over what is left): evA / evB time the whole call
  PinBuf<unsigned char> h_stage;                            // pinned, 2 x 32 MB: result download (qm_fetch_hits)
  // work buffers
  DevBuf<uint32_t> d_cnt; DevBuf<long long> d_offs;         // per unit: hits, exclusive scan
  DevBuf<uint32_t> d_lcnt; DevBuf<long long> d_loff;        // per read: list length / offset
  DevBuf<u64> d_lists;                                      // bump-allocated per-read hit lists
  DevBuf<qm_hit> d_hits;
  DevBuf<u64> d_scal; /* cursor, counters[6], status */ DevBuf<u64> d_gscr; DevBuf<unsigned> d_gslots;   // (scratch slots' flags: gscr_for)
  DevBuf<u64> d_skip;                                       // reads the last call skipped (ReadBatch::skiplist)
  DevBuf<unsigned char> d_scanTmp;                          // (bytes)
  DevBuf<uint8_t> d_seq1, d_seq2; DevBuf<long long> d_off1, d_off2;
  // SA-interval hits as an output (qm_fetch_intervals), foundHit flags, tooMany flags of a merge-only call
  DevBuf<qm_sa_interval_hit> d_iv; DevBuf<uint32_t> d_ivcnt; DevBuf<long long> d_ivoff; int debug = 0;
  DevBuf<unsigned char> d_found, d_tooMany;
  // inputs of the stage entries
  DevBuf<qm_sa_interval_hit> d_ivIn; DevBuf<long long> d_ivInOff; DevBuf<int> d_lenIn;
  // -s (selective alignment) work areas
  DevBuf<unsigned char> d_selscr;
  DevBuf<uint8_t> d_pk1, d_pk2;                             // 2-bit packed reads as uploaded (qm_map_*_packed)
  DevBuf<qm_pack_exc> d_exc1, d_exc2;
  DevBuf<unsigned char> d_kswRows;                          // -s: alignment blocks of the device-memory edition (long reads, band beyond 97)
  DevBuf<long long> d_todoq, d_todoq2;                      // -s: reads the packed list kernel left for the one-read-per-wavefront kernel
  DevBuf<long long> d_slowq;                                // -s slow pass: queue, per-wave scratch descriptors and their memory
  DevBuf<unsigned char> d_dyn, d_dynmem;
  DevBuf<long long> d_toff;
  DevBuf<qm_hit> d_tmp; DevBuf<unsigned char> d_sides; DevBuf<int> d_tsc;
  DevBuf<int> d_tref; DevBuf<u64> d_torder; DevBuf<unsigned char> d_tasks;
  // qm_fetch_stages: CSR offsets of the per-read interval records / list words (scans queued behind stage A), their totals
  // (pinned: they arrive with stage B's synchronisation), the compacted copies
  DevBuf<long long> d_ivcsr, d_lcsr;
  DevBuf<qm_sa_interval_hit> d_ivC; DevBuf<u64> d_wordsC;
  PinBuf<long long> h_tot;
  LastResult last; CallStats stats;                         // what the last call left (begin_call)
  // qm_map_device on a large batch: its parts on helper contexts of the same replica, in flight together (map_device_split)
  uint32_t flags = 0; bool isHelper = false;
  std::vector<qm_ctx*> helpers; struct SplitPool* pool = nullptr;
};

// a few parked threads that run one job per part and call (thread exit in a process with device mappings is slow: they live with the context)
struct SplitPool {
  std::vector<std::thread> th; std::mutex mu; std::condition_variable cv, done;
  std::function<void(int)> job; unsigned long gen = 0; int pending = 0, parts = 0; bool stop = false;
  explicit SplitPool(int n) {
    for (int i = 0; i < n; ++i) th.emplace_back([this, i]() {
      unsigned long seen = 0;
      for (;;) {
        std::function<void(int)> j;
        { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return stop || (gen != seen && i < parts); }); if (stop) return; seen = gen; j = job; }
        j(i);
        { std::lock_guard<std::mutex> lk(mu); if (--pending == 0) done.notify_all(); }
      }
    });
  }
  void run(int n, std::function<void(int)> f) {
    std::unique_lock<std::mutex> lk(mu);
    job = std::move(f); parts = n; pending = n; ++gen;
    cv.notify_all();
    done.wait(lk, [&] { return pending == 0; });
  }
  ~SplitPool() { { std::lock_guard<std::mutex> lk(mu); stop = true; } cv.notify_all(); for (auto& t : th) t.join(); }
};
// where the parts of a split call meet.  The parts finish in order: part p scans its counts from the sum of the totals of the parts
// before it (wait_base), so its offsets are the caller's own, and writes its hits into the caller's array as soon as that array holds
// base + own total records (place: `early`) -- it waits for no part behind it.  The array is grown or replaced only while no write into
// it is in flight: a part that finds it too small waits for every total and for the early writers to finish, the first one through sizes
// the array, and a part that wrote early into the array that was replaced writes again (settle).
struct SplitJoin {
  qm_ctx* owner; int K; std::mutex mu; std::condition_variable cv;
  long long total[8] = {0}, base[9] = {0}; bool have[8] = {false}; int arrived = 0, inflight = 0; bool needGrow = false, sized = false; int failed = 0;
  int wait_base(int part, long long& b);
  int place(int part, long long tot, qm_hit*& dst, bool& early);
  int settle(int part, bool early, bool& again, qm_hit*& dst);
  int failure() { return failed == QM_E_NOMEM ? fail(QM_E_NOMEM, "hipMalloc of the result array failed") : fail(failed, "another part of the batch failed"); }
  void abort(int rc) { std::lock_guard<std::mutex> lk(mu); if (!failed) failed = rc ? rc : QM_E_STATE; cv.notify_all(); }
  // stage A one part after the other (stagger): part i starts its stage A when part i - 1 has finished its own, so that a part's
  // stage A (scalar unit, waiting) runs beside the alignments of the part before it (VALU) instead of beside another stage A
  bool stagger = false; int turn = 0;
  int wait_turn(int part) {
    if (!stagger) return QM_OK;
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return turn >= part || failed; });
    return failed ? fail(failed, "another part of the batch failed") : QM_OK;
  }
  void pass_turn(int part) { if (!stagger) return; std::lock_guard<std::mutex> lk(mu); if (turn < part + 1) turn = part + 1; cv.notify_all(); }
};

// every public entry that maps starts from a clean record
static void begin_call(qm_ctx* c) { c->last.invalidate(); c->stats = CallStats(); }

extern "C" {

const char* qm_last_error(void) { return g_err; }
const char* qm_version(void) { return "qmap_mi355 0.1 (RapMap 0.6.0 quasimap hot path, gfx950)"; }

int qm_opts_default(qm_opts* o) {
  if (!o) return fail(QM_E_ARG, "null opts");
  o->sensitive = 1; o->strict_check = 1; o->max_num_hits = 200; o->no_orphans = 0; o->no_dovetail = 0;
  o->fuzzy = 0; o->max_interval = 1000; o->sel_aln = 0; o->quasi_cov = 0.0;
  o->hard_filter = 0; o->match_score = 2; o->mismatch_penalty = -4; o->gap_open = 4; o->gap_extend = 2; o->dp_bandwidth = 15;
  o->max_mmp_extension = 7; o->aln_policy = 0; o->min_score_fraction = 0.65; o->consensus_slack = 0.2;
  return QM_OK;
}

// --------------------------------------------------------------------------- index
static bool json_field(const std::string& js, const char* name, std::string& out) {
  std::string key = std::string("\"") + name + "\"";
  size_t p = js.find(key);
  if (p == std::string::npos) return false;
  p = js.find(':', p);
  if (p == std::string::npos) return false;
  ++p;
  while (p < js.size() && (js[p] == ' ' || js[p] == '\t' || js[p] == '\n')) ++p;
  size_t e = p;
  if (js[p] == '"') { ++p; e = js.find('"', p); }
  else { while (e < js.size() && js[e] != ',' && js[e] != '\n' && js[e] != '}') ++e; }
  out = js.substr(p, e - p);
  while (!out.empty() && (out.back() == ' ' || out.back() == '\r')) out.pop_back();
  return true;
}

// int64 -> uint32 over a large array (a BigSA index at open), on a few threads; false if a value does not fit
static bool narrow_i64(const uint8_t* src, size_t n, uint32_t* dst) {
  const int nt = n > (1u << 22) ? 16 : 1;
  std::atomic<bool> ok{true};
  auto work = [&](int t) {
    const size_t b = n * (size_t)t / nt, e = n * (size_t)(t + 1) / nt;
    bool good = true;
    for (size_t i = b; i < e; ++i) { int64_t v; memcpy(&v, src + 8 * i, 8); if (v < 0 || v >= 0xffffffffLL) good = false; dst[i] = (uint32_t)v; }
    if (!good) ok = false;
  };
  std::vector<std::thread> th;
  for (int t = 1; t < nt; ++t) th.emplace_back(work, t);
  work(0);
  for (auto& x : th) x.join();
  return ok;
}

int qm_index_open(const char* dirIn, qm_index** out) {
  if (!dirIn || !out) return fail(QM_E_ARG, "null argument");
  qm_index* ix = new qm_index();
  ix->dir = dirIn;
  if (ix->dir.empty() || ix->dir.back() != '/') ix->dir += '/';
  auto bail = [&](int code) { ix->sa.close(); ix->txp.close(); ix->rsd.close(); ix->hash.close(); ix->bph.close(); ix->val.close(); delete ix; return code; };
  {  // header.json (IndexHeader.hpp:45-57)
    FILE* f = fopen((ix->dir + "header.json").c_str(), "rb");
    if (!f) return bail(fail(QM_E_IO, "cannot open %sheader.json", ix->dir.c_str()));
    std::string js; char buf[4096]; size_t r;
    while ((r = fread(buf, 1, sizeof(buf), f)) > 0) js.append(buf, r);
    fclose(f);
    std::string v;
    if (!json_field(js, "KmerLen", v)) return bail(fail(QM_E_IO, "header.json: no KmerLen"));
    ix->k = atoi(v.c_str());
    if (json_field(js, "BigSA", v)) ix->big = (v == "true");
    if (json_field(js, "PerfectHash", v)) ix->perfect = (v == "true");
    if (json_field(js, "IndexVersion", v) && v != "q5") return bail(fail(QM_E_IO, "index version %s != q5", v.c_str()));
    if (ix->k < 1 || ix->k > 31) return bail(fail(QM_E_IO, "bad k %d", ix->k));
  }

  if (ix->sa.open(ix->dir + "sa.bin")) return bail(fail(QM_E_IO, "cannot map sa.bin"));
  if (ix->txp.open(ix->dir + "txpInfo.bin")) return bail(fail(QM_E_IO, "cannot map txpInfo.bin"));
  if (ix->rsd.open(ix->dir + "rsd.bin")) return bail(fail(QM_E_IO, "cannot map rsd.bin"));
  if (!ix->perfect) { if (ix->hash.open(ix->dir + "hash.bin")) return bail(fail(QM_E_IO, "cannot map hash.bin")); }
  else {
    if (ix->bph.open(ix->dir + "hash_info.bph")) return bail(fail(QM_E_IO, "cannot map hash_info.bph"));
    if (ix->val.open(ix->dir + "hash_info.val")) return bail(fail(QM_E_IO, "cannot map hash_info.val"));
  }
  {  // sa.bin: u64 n, n x i32
    const uint8_t* p = (const uint8_t*)ix->sa.p;
    if (ix->sa.len < 8) return bail(fail(QM_E_IO, "sa.bin truncated"));
    uint64_t n; memcpy(&n, p, 8);
    const size_t isz = ix->big ? 8 : 4;
    if (ix->sa.len != 8 + n * isz) return bail(fail(QM_E_IO, "sa.bin size mismatch"));
    // the device's offsets are 32-bit unsigned: a BigSA index fits as long as its text does (0xffffffff is the "none" value)
    if (n >= 0xfffffffeULL) return bail(fail(QM_E_UNSUPPORTED, "text of %llu characters: more than the 2^32 - 2 the device's 32-bit offsets hold", (unsigned long long)n));
    if (ix->big) {
      ix->saNarrow.resize(n);
      if (!narrow_i64(p + 8, n, ix->saNarrow.data())) return bail(fail(QM_E_IO, "sa.bin: entry out of range"));
      ix->SA = ix->saNarrow.data();
    } else ix->SA = (const uint32_t*)(p + 8);
    ix->nSA = (int64_t)n;
  }
  {  // txpInfo.bin: vector<string>, vector<i32>, string(text), vector<u32>
    const uint8_t* p = (const uint8_t*)ix->txp.p; size_t len = ix->txp.len, off = 0;
    auto rd64 = [&](uint64_t& v) { if (off + 8 > len) return false; memcpy(&v, p + off, 8); off += 8; return true; };
    uint64_t cnt;
    if (!rd64(cnt)) return bail(fail(QM_E_IO, "txpInfo.bin truncated"));
    ix->names.reserve(cnt);
    for (uint64_t i = 0; i < cnt; ++i) {
      uint64_t l; if (!rd64(l) || off + l > len) return bail(fail(QM_E_IO, "txpInfo.bin truncated (names)"));
      ix->names.emplace_back((const char*)p + off, (size_t)l); off += l;
    }
    const size_t isz = ix->big ? 8 : 4;                  // vector<int64_t> in a BigSA index (src/RapMapSAIndexer.cpp:711-722)
    uint64_t c2; if (!rd64(c2) || off + c2 * isz > len) return bail(fail(QM_E_IO, "txpInfo.bin truncated (offsets)"));
    if (ix->big) {
      ix->offNarrow.resize(c2);
      if (!narrow_i64(p + off, c2, ix->offNarrow.data())) return bail(fail(QM_E_IO, "txpInfo.bin: offset out of range"));
      ix->offsets = ix->offNarrow.data();
    } else ix->offsets = (const uint32_t*)(p + off);
    ix->nTxp = (int64_t)c2; off += c2 * isz;
    uint64_t tl; if (!rd64(tl) || off + tl > len) return bail(fail(QM_E_IO, "txpInfo.bin truncated (text)"));
    ix->text = p + off; ix->n = (int64_t)tl; off += tl;
    uint64_t c3; if (!rd64(c3) || off + c3 * 4 > len) return bail(fail(QM_E_IO, "txpInfo.bin truncated (lens)"));
    ix->completeLens = (const uint32_t*)(p + off); off += c3 * 4;
    if ((int64_t)cnt != ix->nTxp || ix->nTxp == 0) return bail(fail(QM_E_IO, "txpInfo.bin: name/offset count mismatch"));
    if (ix->n != ix->nSA) return bail(fail(QM_E_IO, "text length %lld != SA length %lld", (long long)ix->n, (long long)ix->nSA));
    // src/RapMapSAIndex.cpp:151-163
    ix->lens.resize(ix->nTxp);
    for (int64_t i = 0; i + 1 < ix->nTxp; ++i) ix->lens[i] = (int64_t)ix->offsets[i + 1] - 1 - ix->offsets[i];
    ix->lens[ix->nTxp - 1] = (ix->nSA - 1) - ix->offsets[ix->nTxp - 1];
  }
  {  // rsd.bin: u64 nbits + bytes (only validated; the device derives transcript ids from the offsets)
    const uint8_t* p = (const uint8_t*)ix->rsd.p;
    if (ix->rsd.len < 8) return bail(fail(QM_E_IO, "rsd.bin truncated"));
    memcpy(&ix->rsdBits, p, 8);
    if (ix->rsd.len != 8 + (ix->rsdBits + 7) / 8) return bail(fail(QM_E_IO, "rsd.bin size mismatch"));
    if ((int64_t)ix->rsdBits != ix->n) return bail(fail(QM_E_IO, "rsd.bin bits != text length"));
  }
  if (ix->perfect) {
    {  // hash_info.bph: boomphf::mphf::save (include/BooPHF.hpp:1172-1197), bitVector::save (:773-781)
      const uint8_t* p = (const uint8_t*)ix->bph.p; size_t len = ix->bph.len, off = 0;
      auto rd = [&](void* d, size_t n) { if (off + n > len) return false; memcpy(d, p + off, n); off += n; return true; };
      double gamma; int32_t nl;
      if (!rd(&gamma, 8) || !rd(&nl, 4) || !rd(&ix->phLastRank, 8) || !rd(&ix->phNelem, 8) || nl < 2 || nl > 64)
        return bail(fail(QM_E_IO, "hash_info.bph truncated"));
      ix->phLevels.resize(nl);
      for (int i = 0; i < nl; ++i) {
        uint64_t size, nchar, nr;
        if (!rd(&size, 8) || !rd(&nchar, 8) || off + nchar * 8 > len) return bail(fail(QM_E_IO, "hash_info.bph truncated (level)"));
        ix->phLevels[i].nchar = nchar; ix->phLevels[i].words = p + off; off += nchar * 8;
        if (!rd(&nr, 8) || off + nr * 8 > len) return bail(fail(QM_E_IO, "hash_info.bph truncated (ranks)"));
        ix->phLevels[i].nranks = nr; ix->phLevels[i].ranks = p + off; off += nr * 8;
      }
      uint64_t fn; if (!rd(&fn, 8) || off + fn * 16 != len) return bail(fail(QM_E_IO, "hash_info.bph size mismatch"));
      for (uint64_t i = 0; i < fn; ++i) { uint64_t kk, vv; rd(&kk, 8); rd(&vv, 8); ix->phFinal.emplace_back(kk, vv); }
      // level domains are not stored: recomputed exactly like mphf::load (:1219-1230)
      double n = (double)ix->phNelem;
      double proba = 1.0 - pow(((gamma * n - 1) / (gamma * n)), (double)ix->phNelem - 1);
      uint64_t hd = (size_t)(ceil(n * gamma));
      for (int i = 0; i < nl; ++i) {
        uint64_t d = (((uint64_t)(hd * pow(proba, i)) + 63) / 64) * 64;
        if (d == 0) d = 64;
        ix->phLevels[i].domain = d;
        if (ix->phLevels[i].nchar < d / 64) return bail(fail(QM_E_IO, "hash_info.bph: level %d smaller than its domain", i));
      }
    }
    {  // hash_info.val: vector<i32> data_, vector<u8> lens_, sparsepp map overflow_ (FrugalBooMap.hpp:199-213)
      const uint8_t* p = (const uint8_t*)ix->val.p; size_t len = ix->val.len, off = 0;
      uint64_t n1, n2;
      if (len < 8) return bail(fail(QM_E_IO, "hash_info.val truncated"));
      memcpy(&n1, p, 8); off = 8;
      const size_t isz = ix->big ? 8 : 4;                // data_ is vector<IndexT>, overflow_ maps IndexT -> IndexT
      if (off + n1 * isz + 8 > len) return bail(fail(QM_E_IO, "hash_info.val truncated (data)"));
      if (ix->big) {
        ix->phDataNarrow.resize(n1);
        if (!narrow_i64(p + off, n1, ix->phDataNarrow.data())) return bail(fail(QM_E_IO, "hash_info.val: entry out of range"));
        ix->phData = (const uint8_t*)ix->phDataNarrow.data();
      } else ix->phData = p + off;
      off += n1 * isz;
      memcpy(&n2, p + off, 8); off += 8;
      if (off + n2 > len || n1 != n2 || n1 != ix->phNelem) return bail(fail(QM_E_IO, "hash_info.val: size mismatch"));
      ix->phLens = p + off; off += n2;
      auto be = [&](uint64_t& v) {
        if (off + 4 > len) return false;
        v = ((uint64_t)p[off] << 24) | ((uint64_t)p[off + 1] << 16) | ((uint64_t)p[off + 2] << 8) | p[off + 3]; off += 4;
        if (v == 0xFFFFFFFFULL) { if (off + 8 > len) return false; v = 0; for (int i = 0; i < 8; ++i) v = (v << 8) | p[off + i]; off += 8; }
        return true;
      };
      uint64_t magic, tsize, nb;
      if (!be(magic) || !be(tsize) || !be(nb) || magic != 0x24687531ULL) return bail(fail(QM_E_IO, "hash_info.val: bad overflow map"));
      off += ((tsize + 31) / 32) * 4;
      if (off + nb * 2 * isz != len) return bail(fail(QM_E_IO, "hash_info.val size mismatch"));
      for (uint64_t i = 0; i < nb; ++i) {
        uint64_t a = 0, b = 0; memcpy(&a, p + off, isz); memcpy(&b, p + off + isz, isz); off += 2 * isz;
        ix->phOverflow.emplace_back((uint32_t)a, (uint32_t)b);
      }
      ix->nKeys = (int64_t)ix->phNelem;
    }
  } else {  // hash.bin: 3 x big-endian u32 (0xFFFFFFFF escapes to u64), group bitmaps, records
    const uint8_t* p = (const uint8_t*)ix->hash.p; size_t len = ix->hash.len, off = 0;
    auto be = [&](uint64_t& v) {
      if (off + 4 > len) return false;
      v = ((uint64_t)p[off] << 24) | ((uint64_t)p[off + 1] << 16) | ((uint64_t)p[off + 2] << 8) | p[off + 3]; off += 4;
      if (v == 0xFFFFFFFFULL) {
        if (off + 8 > len) return false;
        v = 0; for (int i = 0; i < 8; ++i) v = (v << 8) | p[off + i];
        off += 8;
      }
      return true;
    };
    uint64_t magic, tsize, nb;
    if (!be(magic) || !be(tsize) || !be(nb)) return bail(fail(QM_E_IO, "hash.bin truncated"));
    if (magic != 0x24687531ULL) return bail(fail(QM_E_IO, "hash.bin bad magic"));
    off += ((tsize + 31) / 32) * 4;
    const size_t rsz = ix->big ? 24 : 16;                // {u64 key, IndexT begin, IndexT end}
    if (off + nb * rsz != len) return bail(fail(QM_E_IO, "hash.bin size mismatch (%zu + %llu*%zu != %zu)", off, (unsigned long long)nb, rsz, len));
    if (ix->big) {
      ix->hashNarrow.resize(nb * 16);
      for (uint64_t i = 0; i < nb; ++i) {
        const uint8_t* r = p + off + 24 * i; uint8_t* w = ix->hashNarrow.data() + 16 * i;
        int64_t b, e; memcpy(&b, r + 8, 8); memcpy(&e, r + 16, 8);
        if (b < 0 || e < b || e > (int64_t)ix->nSA) return bail(fail(QM_E_IO, "hash.bin: interval out of range"));
        const uint32_t b32 = (uint32_t)b, e32 = (uint32_t)e;
        memcpy(w, r, 8); memcpy(w + 8, &b32, 4); memcpy(w + 12, &e32, 4);
      }
      ix->hashRecs = ix->hashNarrow.data();
    } else ix->hashRecs = p + off;
    ix->nKeys = (int64_t)nb;
  }
  *out = ix;
  return QM_OK;
}

int qm_index_close(qm_index* ix) {
  if (!ix) return QM_OK;
  {   // a later index may be allocated at this address: nothing registered under it may survive it
    std::lock_guard<std::mutex> lk(g_repMu);
    for (auto it = g_reps.begin(); it != g_reps.end();) { if (it->first.first == ix) it = g_reps.erase(it); else ++it; }
    for (auto it = g_repBuild.begin(); it != g_repBuild.end();) { if (it->first.first == ix) it = g_repBuild.erase(it); else ++it; }
  }
  ix->sa.close(); ix->txp.close(); ix->rsd.close(); ix->hash.close(); ix->bph.close(); ix->val.close();
  delete ix;
  return QM_OK;
}

int qm_index_info_get(const qm_index* ix, qm_index_info* info) {
  if (!ix || !info) return fail(QM_E_ARG, "null argument");
  info->k = ix->k; info->big_sa = ix->big; info->perfect_hash = ix->perfect; info->pad = 0;
  info->text_len = ix->n; info->n_txps = ix->nTxp; info->n_keys = ix->nKeys;
  return QM_OK;
}
const char* qm_index_txp_name(const qm_index* ix, int64_t tid) {
  if (!ix || tid < 0 || tid >= ix->nTxp) return nullptr;
  return ix->names[tid].c_str();
}
int64_t qm_index_txp_len(const qm_index* ix, int64_t tid) {
  if (!ix || tid < 0 || tid >= ix->nTxp) return -1;
  return ix->lens[tid];
}

int qm_index_arrays(const qm_index* ix, const uint8_t** text, int64_t* text_len, const int32_t** txp_offsets,
                    int64_t* n_txps) {
  if (!ix) return fail(QM_E_ARG, "null index");
  if (text) *text = ix->text;
  if (text_len) *text_len = ix->n;
  if (txp_offsets) *txp_offsets = (const int32_t*)ix->offsets;      // unsigned values for a BigSA index
  if (n_txps) *n_txps = ix->nTxp;
  return QM_OK;
}

int qm_index_raw(const qm_index* ix, int which, const void** data, int64_t* count) {
  if (!ix || !data || !count) return fail(QM_E_ARG, "null argument");
  switch (which) {
    case QM_RAW_SA: *data = ix->SA; *count = ix->nSA; break;
    case QM_RAW_HASH: *data = ix->perfect ? nullptr : ix->hashRecs; *count = ix->perfect ? 0 : ix->nKeys; break;
    case QM_RAW_COMPLETE_LENS: *data = ix->completeLens; *count = ix->nTxp; break;
    default: return fail(QM_E_ARG, "qm_index_raw: unknown array %d", which);
  }
  return QM_OK;
}

// --------------------------------------------------------------------------- context
int qm_ctx_destroy(qm_ctx* c) {
  if (!c) return QM_OK;
  hipSetDevice(c->device);
  delete c->pool; c->pool = nullptr;
  for (qm_ctx* h : c->helpers) qm_ctx_destroy(h);
  c->helpers.clear();
  if (c->stream) hipStreamDestroy(c->stream);
  if (c->copyStream) hipStreamDestroy(c->copyStream);
  if (c->planStream) hipStreamDestroy(c->planStream);
  hipEvent_t evs[] = {c->ev0, c->ev1, c->evA, c->evB, c->evCopy, c->evP0, c->evP1, c->evStage[0], c->evStage[1]};
  for (hipEvent_t e : evs) if (e) hipEventDestroy(e);
  for (hipEvent_t e : c->evPlan) if (e) hipEventDestroy(e);
  {   // the last context on (index, device) frees the replica
    std::lock_guard<std::mutex> lk(g_repMu);
    c->rep.reset();
    for (auto it = g_reps.begin(); it != g_reps.end();) { if (it->second.expired()) it = g_reps.erase(it); else ++it; }
  }
  delete c;                    // (the work buffers free themselves)
  return QM_OK;
}

int qm_ctx_create(const qm_index* ix, int device_id, qm_ctx** out) { return qm_ctx_create_ex(ix, device_id, 0, out); }

static bool ensure_saext2(qm_ctx* c);
static int build_replica(const qm_index* ix, int device, bool phCompact, hipStream_t stream, Replica& R);
int qm_ctx_create_ex(const qm_index* ix, int device_id, uint32_t flags, qm_ctx** out) {
  if (!ix || !out) return fail(QM_E_ARG, "null argument");
  const bool phCompact = ix->perfect && (flags & QM_CTX_PH_COMPACT);
  const int repKey = device_id * 2 + (phCompact ? 1 : 0);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(QM_E_NOGPU, "no HIP device visible");
  if (device_id < 0 || device_id >= ndev) return fail(QM_E_ARG, "device %d out of range (%d devices)", device_id, ndev);
  HIPCHK(hipSetDevice(device_id));
  qm_ctx* c = new qm_ctx();
  c->ix = ix; c->device = device_id; c->flags = flags;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) c->numCU = prop.multiProcessorCount;
  int rc;
#define CK(x) do { hipError_t _e = (x); if (_e != hipSuccess) { rc = fail(QM_E_NOGPU, "%s: %s", #x, hipGetErrorString(_e)); qm_ctx_destroy(c); return rc; } } while (0)
  CK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  CK(hipStreamCreateWithFlags(&c->copyStream, hipStreamNonBlocking));
  CK(hipStreamCreateWithFlags(&c->planStream, hipStreamNonBlocking));
  for (hipEvent_t& e : c->evPlan) CK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  CK(hipEventCreateWithFlags(&c->evCopy, hipEventDisableTiming));
  CK(hipEventCreate(&c->ev0)); CK(hipEventCreate(&c->ev1)); CK(hipEventCreate(&c->evA)); CK(hipEventCreate(&c->evB));
  CK(hipEventCreate(&c->evP0)); CK(hipEventCreate(&c->evP1));
#undef CK
  if ((rc = c->d_ntk.ensure(3 * QM_SEL_CHUNKS_B)) || (rc = c->d_scal.ensure(QM_SC_WORDS)) || (rc = c->d_skip.ensure(QM_SKIP_CAP))) { qm_ctx_destroy(c); return rc; }
  // one builder per (index, device image) at a time: a second thread that asks for the same replica while the first one is
  // still uploading waits here and then shares it
  std::shared_ptr<std::mutex> buildMu;
  {
    std::lock_guard<std::mutex> lk(g_repMu);
    auto& m = g_repBuild[std::make_pair(ix, repKey)];
    if (!m) m = std::make_shared<std::mutex>();
    buildMu = m;
  }
  std::lock_guard<std::mutex> buildLock(*buildMu);
  {
    std::lock_guard<std::mutex> lk(g_repMu);
    auto it = g_reps.find(std::make_pair(ix, repKey));
    if (it != g_reps.end()) c->rep = it->second.lock();
  }
  if (!c->rep) {
    auto R = std::make_shared<Replica>();
    if ((rc = build_replica(ix, device_id, phCompact, c->stream, *R))) { R.reset(); qm_ctx_destroy(c); return rc; }
    std::lock_guard<std::mutex> lk(g_repMu);
    c->rep = R;
    g_reps[std::make_pair(ix, repKey)] = R;
  }
  { std::lock_guard<std::mutex> lk(c->rep->sanextMu); c->d_sanext = c->rep->sanext; c->devBytes = c->rep->devBytes; }
  // the wide extension table with the replica when the caller knows reads of 129 .. 256 characters are coming: otherwise the first call
  // that has such reads builds it (0.2 s for config 2) inside that call (a replica without room for it goes on with the general kernels)
  if (flags & QM_CTX_WIDE_READS) (void)ensure_saext2(c);
  *out = c;
  return QM_OK;
}

// The device image of an index, built into R on `stream`.  On an error R is left as far as it got: it frees what it holds.
static int build_replica(const qm_index* ix, int device, bool phCompact, hipStream_t stream, Replica& R) {
  int rc;
  R.device = device;
  const size_t pad = 256;
  if ((rc = R.text.ensure(ix->n + (int64_t)pad))) return rc;
  HIPCHK(hipMemsetAsync(R.text + ix->n, 0, pad, stream));
  HIPCHK(hipMemcpyAsync(R.text, ix->text, (size_t)ix->n, hipMemcpyHostToDevice, stream));
  if ((rc = R.SA.ensure(ix->nSA))) return rc;
  HIPCHK(hipMemcpyAsync(R.SA, ix->SA, (size_t)ix->nSA * 4, hipMemcpyHostToDevice, stream));
  if ((rc = R.sainfo.ensure(ix->nSA * (int64_t)sizeof(SaInfo)))) return rc;
  if ((rc = R.txpOff.ensure(ix->nTxp))) return rc;      // kept: -s reads transcript sequences by (offset, length)
  HIPCHK(hipMemcpyAsync(R.txpOff, ix->offsets, (size_t)ix->nTxp * 4, hipMemcpyHostToDevice, stream));
  HIPCHK(qmk_build_sainfo(R.SA, ix->nSA, R.txpOff, ix->nTxp, R.sainfo, stream));
  if (!getenv("QM_NO_SAEXT") && ix->nSA > 0 && ix->nTxp < (1LL << QM_EXT_TID_BITS)) {
    // the packed characters behind every suffix's k-mer: an MMP extension becomes one trip instead of two (saext_entry);
    // 32 bytes per suffix-array entry.  QM_NO_SAEXT (profiling): without the table, extensions read suffix array and text.
    if (R.saext.ensure(ix->nSA * (int64_t)sizeof(SaExt))) (void)hipGetLastError();   // no room: the text path
    else HIPCHK(qmk_build_saext(R.text, ix->n, R.SA, ix->nSA, ix->k, R.sainfo, R.saext, stream));
  }
  DevBuf<unsigned char> recs;                              // staging: the hash records as the file has them
  if (!ix->perfect) {
    R.cap = bucket_count(ix->nKeys);                  // 64-byte buckets of two canonical entries, at least two buckets per key
    if ((rc = R.slots.ensure((int64_t)(R.cap * sizeof(Bucket))))) return rc;
    if ((rc = recs.ensure((ix->nKeys > 0 ? ix->nKeys : 1) * 16))) return rc;
    if (ix->nKeys > 0) HIPCHK(hipMemcpyAsync(recs, ix->hashRecs, (size_t)ix->nKeys * 16, hipMemcpyHostToDevice, stream));
    HIPCHK(qmk_build_slots(recs, ix->nKeys, R.slots, R.cap, ix->k, stream));
  } else {
    // flatten BooPHF + FrugalBooMap: all levels' words / rank samples concatenated, small maps re-hashed
    R.cap = 1;
    PhIndex P; memset(&P, 0, sizeof(P));
    const int nl = (int)ix->phLevels.size();
    std::vector<PhLevelIn> lin((size_t)nl);
    for (int i = 0; i < nl; ++i) {
      lin[i].words = (const uint64_t*)ix->phLevels[i].words; lin[i].nchar = ix->phLevels[i].nchar; lin[i].domain = ix->phLevels[i].domain;
      lin[i].ranks = (const uint64_t*)ix->phLevels[i].ranks; lin[i].nranks = ix->phLevels[i].nranks;
    }
    std::vector<uint64_t> blocks, tab;
    if (!ph_flatten_blocks(lin, blocks, tab)) return fail(QM_E_IO, "hash_info.bph: rank samples do not match the bit arrays");
    auto dalloc = [&](size_t bytes) -> void* { DevBuf<unsigned char>& q = R.phAllocs.emplace_back(); if (q.ensure((int64_t)(bytes ? bytes : 16))) return nullptr; R.devBytes += (int64_t)bytes; return q.p; };
    u64* dW = (u64*)dalloc(blocks.size() * 8); u64* dT = (u64*)dalloc(tab.size() * 8);
    PhRec* dRec = (PhRec*)dalloc((size_t)ix->phNelem * sizeof(PhRec));
    DevBuf<unsigned int> dD; DevBuf<unsigned char> dL;       // staging for the record builder
    if (dD.ensure((int64_t)(ix->phNelem ? ix->phNelem : 1)) || dL.ensure((int64_t)(ix->phNelem ? ix->phNelem : 1)) || !dW || !dT || !dRec) return fail(QM_E_NOMEM, "hipMalloc (perfect hash) failed");
    HIPCHK(hipMemcpyAsync(dW, blocks.data(), blocks.size() * 8, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(dT, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(dD, ix->phData, (size_t)ix->phNelem * 4, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(dL, ix->phLens, (size_t)ix->phNelem, hipMemcpyHostToDevice, stream));
    {
      DevIndex dix; memset(&dix, 0, sizeof(dix));
      dix.text = R.text; dix.n = ix->n; dix.SA = R.SA; dix.nSA = ix->nSA; dix.k = ix->k;
      HIPCHK(qmk_build_phrecs(dD, dL, ix->phNelem, dix, dRec, stream));
      HIPCHK(hipStreamSynchronize(stream));
      dD.release(); dL.release();
    }
    auto mix = [](u64 x) { x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33; return x; };
    std::vector<OvfSlot> ov; std::vector<Slot> fin;
    {
      u64 cap = 16; while (cap < ix->phOverflow.size() * 2) cap <<= 1;
      ov.assign(cap, OvfSlot{~0u, 0u});
      for (auto& kv : ix->phOverflow) { u64 j = mix((u64)kv.first) & (cap - 1); while (ov[j].key != ~0u) j = (j + 1) & (cap - 1); ov[j].key = kv.first; ov[j].val = kv.second; }
      P.ovfMask = cap - 1;
      u64 fc = 16; while (fc < ix->phFinal.size() * 2) fc <<= 1;
      Slot e; e.key = ~0ULL; e.lb = 0; e.ub = 0;
      fin.assign(fc, e);
      for (auto& kv : ix->phFinal) { u64 j = mix(kv.first) & (fc - 1); while (fin[j].key != ~0ULL) j = (j + 1) & (fc - 1); fin[j].key = kv.first; fin[j].lb = (int)kv.second; }
      P.finMask = fc - 1;
    }
    OvfSlot* dO = (OvfSlot*)dalloc(ov.size() * sizeof(OvfSlot)); Slot* dF = (Slot*)dalloc(fin.size() * sizeof(Slot));
    void* dP = dalloc(sizeof(PhIndex));
    if (!dO || !dF || !dP) return fail(QM_E_NOMEM, "hipMalloc (perfect hash) failed");
    HIPCHK(hipMemcpyAsync(dO, ov.data(), ov.size() * sizeof(OvfSlot), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(dF, fin.data(), fin.size() * sizeof(Slot), hipMemcpyHostToDevice, stream));
    P.blocks = dW; P.levelTab = dT; P.recs = dRec; P.ovf = dO; P.fin = dF;
    P.lastbitsetrank = ix->phLastRank; P.nelem = ix->phNelem; P.nb_levels = nl;
    if (phCompact && !getenv("QM_PH_NO_FILTER")) {
      // the membership pre-filter of the compact image (PhIndex::filter): absent k-mers -- most lookups -- are rejected after
      // one sector instead of a walk through the levels.  QM_PH_NO_FILTER (profiling): the bare reference structure.
      const u64 fw = ph_filter_words(ix->phNelem);
      u64* dFil = (u64*)dalloc(fw * 8);
      if (!dFil) return fail(QM_E_NOMEM, "hipMalloc (perfect hash filter) failed");
      HIPCHK(hipMemsetAsync(dFil, 0, fw * 8, stream));
      HIPCHK(qmk_build_phfilter(dRec, (long long)ix->phNelem, dFil, fw - 1, ix->k, stream));
      P.filter = dFil; P.filterMask = fw - 1;
    }
    HIPCHK(hipMemcpyAsync(dP, &P, sizeof(P), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));    // P, tab, ov, fin are locals
    R.ph = (const PhIndex*)dP; R.hPh = P;
    if (!phCompact) {
      // Default device image of a -p index: the same one-sector bucket table a dense index gets, filled from the MPHF's own
      // records after each was looked up through the BooPHF walk (so the table is known to answer like FrugalBooMap::find on
      // this file).  288 GB of HBM make the frugal structure unnecessary on this device; QM_CTX_PH_COMPACT keeps it.
      R.cap = bucket_count((long long)ix->phNelem);
      DevBuf<unsigned long long> dBad; unsigned long long hBad = 0;
      if ((rc = R.slots.ensure((int64_t)(R.cap * sizeof(Bucket)))) || (rc = dBad.ensure(1))) return rc;
      DevIndex dix; memset(&dix, 0, sizeof(dix));
      dix.text = R.text; dix.n = ix->n; dix.SA = R.SA; dix.nSA = ix->nSA; dix.k = ix->k; dix.ph = R.ph; dix.phv = P;
      HIPCHK(qmk_build_slots_from_ph(dix, (long long)ix->phNelem, R.slots, R.cap, dBad, stream));
      HIPCHK(hipMemcpyAsync(&hBad, dBad, sizeof(hBad), hipMemcpyDeviceToHost, stream));
      HIPCHK(hipStreamSynchronize(stream));
      if (hBad) return fail(QM_E_IO, "hash_info.bph / hash_info.val: %llu k-mers are not found by the perfect hash they were stored with", hBad);
      R.phAllocs.clear(); R.ph = nullptr; R.devBytes = (int64_t)(R.cap * sizeof(Bucket));
    }
  }
  HIPCHK(hipStreamSynchronize(stream));
  {
    std::vector<int32_t> l32((size_t)ix->nTxp);
    for (int64_t t = 0; t < ix->nTxp; ++t) l32[(size_t)t] = (int32_t)ix->lens[(size_t)t];
    if ((rc = R.txpLen.ensure(ix->nTxp ? ix->nTxp : 1))) return rc;
    HIPCHK(hipMemcpy(R.txpLen, l32.data(), (size_t)ix->nTxp * 4, hipMemcpyHostToDevice));
  }
  R.devBytes += ix->n + pad + ix->nSA * 4 + ix->nSA * (int64_t)sizeof(SaInfo) + (int64_t)(ix->perfect ? 0 : R.cap * sizeof(Bucket))
                + (R.saext ? ix->nSA * (int64_t)sizeof(SaExt) : 0);
  return QM_OK;
}

int64_t qm_ctx_device_bytes(const qm_ctx* c) { return c ? c->devBytes : 0; }
int qm_ctx_set_debug(qm_ctx* c, int keep) { if (!c) return fail(QM_E_ARG, "null ctx"); c->debug = keep; return QM_OK; }

static int check_opts(const qm_opts* o) {
  if (!o) return fail(QM_E_ARG, "null opts");
  if (o->max_num_hits < 0 || o->max_interval < 1) return fail(QM_E_ARG, "bad max_num_hits / max_interval");
  return QM_OK;
}

// Host-buffer callers (qm_map_pairs / qm_map_reads) hand stage A its input chunk by chunk: `upload(u0, u1)` queues the
// characters of units [u0, u1) on the copy stream, the kernel for those units waits for that copy only, so the upload of
// chunk i + 1 runs under the kernel of chunk i.  Device-buffer callers pass no feeder: one launch over everything.
struct ChunkFeeder {
  int64_t chunk;                                             // units per chunk
  int (*upload)(void* self, int64_t u0, int64_t u1);         // QM_OK or an error code (already recorded with fail())
  void* self;
};

// What a call asks of the path.  The fused calls (qm_map_pairs / _reads / _device) run everything; the stage entries run one
// of the reference's three entry points on its own (SACollector::operator(), hitsToMappingsSimple, mergeLeftRightHits[Fuzzy]).
enum { QM_RUN_FUSED = 0, QM_RUN_COLLECT = 1, QM_RUN_FROM_INTERVALS = 2 };
struct RunReq {
  int mode = QM_RUN_FUSED;
  bool keepIntervals = false;     // SA-interval hits kept for qm_fetch_intervals
  bool keepFound = false;         // foundHit per read kept for qm_fetch_found
  bool mergeOnly = false;         // stage B without the caller-level bookkeeping, tooMany flags kept
  bool stageView = false;         // qm_map_pairs_stages: queue the CSR scans of the per-read outputs behind stage A (qm_fetch_stages)
  bool longReads = false;         // the batch holds reads beyond QM_MAX_READ_LEN (set by map_device_impl from max_read_len)
  int shortLen = 0;               // the longest read that is not beyond QM_MAX_READ_LEN (0: unknown)
  // QM_RUN_FROM_INTERVALS: device arrays
  const qm_sa_interval_hit* ivIn = nullptr; const long long* ivInOff = nullptr; const int* lenIn = nullptr; const unsigned char* foundIn = nullptr;
  SplitJoin* join = nullptr; int part = 0; int64_t u0 = 0;   // one part of a split call (map_device_split), units u0 .. of the batch: hits and offsets go to the caller's arrays
  bool noDuo = false;             // this part takes qm_lean_kernel even where the pair kernel could (map_device_split: parts of both kinds in flight)
};

static DevIndex dev_index(const qm_ctx* c) {
  const Replica& R = *c->rep;
  DevIndex ix; ix.text = R.text; ix.n = c->ix->n; ix.SA = R.SA; ix.nSA = c->ix->nSA;
  ix.sainfo = (const SaInfo*)R.sainfo.p; ix.slots = (const Bucket*)R.slots.p; ix.hmask = R.cap - 1; ix.ph = R.ph; ix.k = c->ix->k;
  memset(&ix.phv, 0, sizeof(ix.phv)); if (R.ph) ix.phv = R.hPh;
  ix.sanext = c->d_sanext; ix.saext = (const SaExt*)R.saext.p; ix.saext2 = (const SaExt2*)c->d_saext2;
  return ix;
}

// ---- stage A: one wavefront per read (collector + hits->mappings, or one of the two alone), with its retries: the per-read
// lists or the interval output outgrew their buffers (grow, redo), -s reads left on the slow queue (second, small launch).
// The longest read a call takes is QM_MAX_LONG_READ_LEN, with -s too, whatever the band: a --dpBandwidth beyond 97 takes the
// device-memory edition of the alignment kernel.

// The wide extension table (SaExt2: 224 characters behind every suffix's k-mer, 64 bytes per suffix-array entry) for the one-read-per-
// wavefront lean kernel: built by the first call that has reads of 129 .. 256 characters, shared by the replica's contexts; a replica
// that has no room for it (or no SaExt) goes on with the general kernels.  So does an index of 2^QM_EXT2_TID_BITS transcripts or more:
// the limit comes from the entry layout (saext2_entry keeps the transcript in that many bits, one fewer than SaExt's), so SaExt being
// there does not imply it.
static bool ensure_saext2(qm_ctx* c) {
  if (c->d_saext2) return true;
  Replica& R = *c->rep;
  if (!R.saext || c->ix->nSA <= 0 || c->ix->nTxp >= (1LL << QM_EXT2_TID_BITS)) return false;
  std::lock_guard<std::mutex> lk(R.sanextMu);
  if (!R.saext2 && !R.saext2Tried) {
    R.saext2Tried = true;
    // room for the table AND a margin for the work buffers of the replica's contexts (lists, hits, scratch: they grow with the batches);
    // a replica that cannot spare it stays with the general kernels for such reads
    size_t freeB = 0, totalB = 0;
    const size_t need = (size_t)c->ix->nSA * sizeof(SaExt2), margin = (size_t)8 << 30;
    if (hipMemGetInfo(&freeB, &totalB) != hipSuccess || freeB < need + margin) { (void)hipGetLastError(); return false; }
    if (R.saext2.ensure((int64_t)need)) { (void)hipGetLastError(); return false; }
    hipError_t e = qmk_build_saext2(R.text, c->ix->n, R.SA, c->ix->nSA, c->ix->k, R.sainfo, R.saext2, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { R.saext2.release(); (void)hipGetLastError(); return false; }
    R.devBytes += c->ix->nSA * (int64_t)sizeof(SaExt2);
  }
  c->d_saext2 = R.saext2; c->devBytes = R.devBytes;
  return c->d_saext2 != nullptr;
}

// The -s extension table (sanext_entry: a capped MMP extension becomes one trip; 4 bytes per suffix-array entry, built from text and SA as
// they sit in HBM): built by the first -s call on a replica, shared by every context of the replica.
static int ensure_sanext(qm_ctx* c) {
  if (c->d_sanext || c->ix->nSA <= 0) return QM_OK;
  Replica& R = *c->rep;
  std::lock_guard<std::mutex> lk(R.sanextMu);
  if (!R.sanext) {
    if (int rc = R.sanext.ensure(c->ix->nSA)) return rc;
    hipError_t e = qmk_build_sanext(R.text, c->ix->n, R.SA, c->ix->nSA, c->ix->k, R.sanext, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { R.sanext.release(); return fail(QM_E_NOGPU, "building the -s extension table: %s", hipGetErrorString(e)); }
    R.devBytes += c->ix->nSA * 4;
  }
  c->d_sanext = R.sanext; c->devBytes = R.devBytes;
  return QM_OK;
}

// The general kernels' per-wave scratch in device memory (QM_GSCR_U64 words, 112 KB) for a launch of `grid` blocks: one per launched
// wave while that is no more than the waves that can be resident at once (64 per CU, generously); beyond that -- the oversubscribed
// grids -- one per SLOT, and the waves take and return slots as they start and end (ReadBatch::gslots).  Returns the flags, or null.
// XCDs of the device a context launches on: 32 CUs each on gfx950 (a whole MI355X: 8; its DPX / QPX / CPX partitions: 4 / 2 / 1)
static int xcds_of(const qm_ctx* c) { const int x = c->numCU / 32; return x < 1 ? 1 : (x > 8 ? 8 : x); }
static int gscr_for(qm_ctx* c, int grid, unsigned*& slots, int& nslots) {
  // (64 slots per CU = 2 048 per XCD of 32 CUs, twice the 1 024 wavefronts that can be resident there, whatever the partition)
  const int64_t waves = (int64_t)grid * 4, cap = (int64_t)c->numCU * 64;
  slots = nullptr; nslots = 0;
  const char* fe = getenv("QM_GSCR_SLOTS");                  // (tests: slots for launches that would not need them)
  const bool force = fe && atoi(fe) != 0;
  int rc = c->d_gscr.ensure((waves > cap || force ? cap : waves) * QM_GSCR_U64);
  if (rc || (waves <= cap && !force)) return rc;
  if ((rc = c->d_gslots.ensure(cap))) return rc;
  HIPCHK(hipMemsetAsync(c->d_gslots, 0, (size_t)cap * sizeof(unsigned), c->stream));
  slots = c->d_gslots; nslots = (int)cap;
  return QM_OK;
}

// What a call of stage A runs, decided once (plan_stage_a): which kernels, over what grid, writing which outputs.
enum { SK_GENERAL, SK_LEAN, SK_DUO, SK_LEAN_SEL, SK_H2M };
struct StagePlan {
  int first;                // the first launch.  SK_GENERAL: the general kernels (fused, or the collector alone: QM_RUN_COLLECT, the first half of twoPass); SK_LEAN: qm_lean_kernel;
                            // SK_DUO: the pair kernel; SK_LEAN_SEL: qm_lean_kernel's -s edition as the collector of twoPass; SK_H2M: hits -> mappings alone (QM_RUN_FROM_INTERVALS)
  bool leanWide, duoMerge;  // the lean kernels' one-read-per-wavefront edition (reads of 129 .. 256 characters); the pair kernel merges the pairs it maps (pair_cnt)
  bool twoPass, wantIv, wantFound;   // fused -s: a collector, then the list kernels; the SA-interval records / the foundHit flags are written
  bool paired; int ns, phc; int64_t n, nreads;
  int grid; unsigned* gslots; int ngslots;   // blocks of a launch of the general kernels over the whole batch (reserve_stage_a lowers it when their scratch does not fit) and the flags of their scratch slots, if any (gscr_for)
};
static bool lean_first(const StagePlan& p) { return p.first == SK_LEAN || p.first == SK_DUO; }   // the fused default call: lists from a kernel that owns no scratch in device memory

static int plan_stage_a(qm_ctx* c, const qm_opts* o, const RunReq& rq, bool paired, int64_t n, int ns, StagePlan& p) {
  p.paired = paired; p.n = n; p.nreads = paired ? 2 * n : n; p.ns = ns;
  p.phc = c->rep->ph ? 1 : 0;                                // (the compact -p image: its kernels take a larger grid)
  p.grid = map_grid(p.nreads, c->numCU, p.phc); p.gslots = nullptr; p.ngslots = 0;
  // The lean kernel (qm_lean.inl: two reads per wavefront and iteration, reads of up to 128 clean characters) takes the fused default
  // call on a dense table; the reads it marks instead of mapping go through the general kernel in a second, small launch (pass_lean_leftovers).
  // It owns no per-wave scratch in device memory: that is only reserved -- for the small grid -- when the second launch happens.
  static const bool leanOff = [] { const char* e = getenv("QM_NO_LEAN"); return e && atoi(e) != 0; }();
  // Reads of 129 .. 256 characters (slot classes 3 and 4) take its wide edition -- one read per wavefront -- once the replica holds the
  // wide extension table.
  static const bool wideOff = [] { const char* e = getenv("QM_NO_LEAN_WIDE"); return e && atoi(e) != 0; }();
  const bool leanBase = !leanOff && rq.mode == QM_RUN_FUSED && o->sensitive && (c->rep->slots || c->rep->ph) && c->rep->saext && c->ix->k <= 31;
  // (a call that keeps the SA-interval records takes the general kernel: the lean kernels do not write them; foundHit they do -- stage views without intervals)
  p.leanWide = leanBase && !wideOff && (ns == 3 || ns == 4) && (o->sel_aln || !rq.keepIntervals) && ensure_saext2(c);
  const bool useLean = leanBase && !o->sel_aln && (ns == 2 || p.leanWide) && !rq.keepIntervals;
  // Pairs of such reads take the pair kernel (qm_duo.inl): the two mates walked in lockstep by the two halves of a wavefront, and -- in a
  // plain fused call -- merged there (pair_cnt: stage B's count pass finds the pair done, its write pass expands the records)
  static const bool duoOff = [] { const char* e = getenv("QM_NO_DUO"); return e && atoi(e) != 0; }();
  // (dense table only: on the compact -p image a position's two orientations are two walks of the BooPHF levels, and a lane per position
  // serialises them -- 301 M pairs/s against qm_lean_kernel's 323, profiles/r06/exp_mix.txt)
  static const bool duoPh = [] { const char* e = getenv("QM_DUO_PH"); return e && atoi(e) != 0; }();
  const bool useDuo = useLean && !duoOff && !rq.noDuo && !(c->flags & QM_CTX_NO_PAIR_KERNEL) && paired && ns == 2 && (!c->rep->ph || duoPh);
  // (qm_lean_kernel holds both mates of a pair in one wavefront too, but merging there was measured and dropped: that kernel is bound by the CU's scalar unit and
  // the merge's bookkeeping cost it 1.3 ms per 10 M pairs -- 62 instead of 28 spilled scalar registers -- where stage B saved 0.5: profiles/r06/exp_mix.txt)
  p.duoMerge = useDuo && !rq.mergeOnly && !rq.stageView;
  // A fused -s call runs stage A as two launches: the chain-scoring collector alone (its memory-bound walk, at the default
  // kernel's occupancy: without the chaining code it needs half the registers and no LDS scratch) leaves every read's
  // SA-interval hits in HBM, then one wavefront per read turns them into the read's list (sort, slack intersection, chaining).
  p.twoPass = rq.mode == QM_RUN_FUSED && o->sel_aln != 0;
  p.wantIv = rq.keepIntervals || rq.mode == QM_RUN_COLLECT || p.twoPass;
  p.wantFound = rq.keepFound || rq.mode == QM_RUN_COLLECT || p.twoPass;
  // ... and the lean kernel's -s edition stands in for that collector (intervals and foundHit out; the list kernels that follow are the same); every collector of a -s call reads the -s extension table
  if (o->sel_aln && rq.mode != QM_RUN_FROM_INTERVALS) { const int rc = ensure_sanext(c); if (rc) return rc; }
  const bool useLeanSel = leanBase && o->sel_aln && (ns == 2 || p.leanWide) && c->d_sanext;
  p.first = useDuo ? SK_DUO : useLean ? SK_LEAN : useLeanSel ? SK_LEAN_SEL : rq.mode == QM_RUN_FROM_INTERVALS ? SK_H2M : SK_GENERAL;
  return QM_OK;
}

// The work buffers of a call, sized from the plan.
static int reserve_stage_a(qm_ctx* c, const qm_opts* o, const RunReq& rq, StagePlan& p) {
  int rc;
  if ((rc = c->d_lcnt.ensure(p.nreads + 1))) return rc;
  if ((rc = c->d_loff.ensure(p.nreads + 1))) return rc;
  if (p.duoMerge && (rc = c->d_cnt.ensure(p.n + 1))) return rc;
  if (!lean_first(p)) {
    // the general kernels' scratch (gscr_for); when even that does not fit next to the index, the launch falls back to the resident grid
    rc = gscr_for(c, p.grid, p.gslots, p.ngslots);
    if (rc == QM_E_NOMEM) { p.grid = resident_grid(p.nreads, c->numCU); rc = gscr_for(c, p.grid, p.gslots, p.ngslots); }
    if (rc) return rc;
  }
  // lists and interval records come from chunked bump allocators: up to one open chunk per wave
  if (rq.mode != QM_RUN_COLLECT && (rc = c->d_lists.ensure(p.nreads * 4 + (int64_t)p.grid * 4 * QM_CHUNK * 2))) return rc;
  if (p.wantIv) {
    if ((rc = c->d_ivcnt.ensure(p.nreads + 1))) return rc;
    if ((rc = c->d_ivoff.ensure(p.nreads + 1))) return rc;
    if ((rc = c->d_iv.ensure(p.nreads * (o->sel_aln ? 16 : 4) + (int64_t)p.grid * 4 * QM_IVCHUNK * 2))) return rc;
  }
  if (p.wantFound && (rc = c->d_found.ensure(p.nreads + 1))) return rc;
  // -s: per-wave scratch for chaining (qm_sel.inl; the list kernels' grids stay within residency)
  if (o->sel_aln && (rc = c->d_selscr.ensure((int64_t)resident_grid(p.nreads, c->numCU) * 4 * (int64_t)sizeof(SelScratch)))) return rc;
  return QM_OK;
}

// The first launch's view of the batch; the follow-up passes copy it and point the copy at their queue.
static void fill_batch(const qm_ctx* c, const qm_opts* o, const RunReq& rq, const StagePlan& p, const void* d_seq1, const void* d_off1,
                       const void* d_seq2, const void* d_off2, ReadBatch& B) {
  memset(&B, 0, sizeof(B));
  B.seq1 = (const unsigned char*)d_seq1; B.off1 = (const long long*)d_off1;
  B.seq2 = (const unsigned char*)d_seq2; B.off2 = (const long long*)d_off2; B.nreads = p.nreads;
  B.lcnt = c->d_lcnt; B.loff = c->d_loff; B.lists = c->d_lists; B.cursor = c->d_scal; B.lists_cap = c->d_lists.cap;
  B.status = (int*)(c->d_scal + QM_SC_STATUS); B.gscratch = c->d_gscr; B.gslots = p.gslots; B.ngslots = p.ngslots; B.gxcd = xcds_of(c); B.skiplist = c->d_skip;
  B.lean_wide = p.leanWide ? 1 : 0;
  if (p.duoMerge) { B.pair_cnt = c->d_cnt; B.max_num_hits = o->max_num_hits; B.no_orphans = o->no_orphans; B.no_dovetail = o->no_dovetail; }
  if (p.wantIv) { B.iv_out = c->d_iv; B.iv_cnt = c->d_ivcnt; B.iv_off = c->d_ivoff; B.iv_cap = c->d_iv.cap; }
  if (p.wantFound) B.found_out = c->d_found;
  B.iv_in = rq.ivIn; B.iv_in_off = rq.ivInOff; B.len_in = rq.lenIn; B.found_in = rq.foundIn;
  B.strict_check = o->strict_check; B.max_interval = o->max_interval; B.quasi_cov = o->quasi_cov; B.sensitive = o->sensitive; B.fuzzy = p.paired ? o->fuzzy : 0;
  if (rq.mode == QM_RUN_FROM_INTERVALS) B.fuzzy = o->fuzzy;   // the caller says what kind of list it wants (both orientations kept or not)
  if (o->sel_aln) {                                   // -s: chain scoring + per-wave scratch for chaining (qm_sel.inl)
    B.selscr = (SelScratch*)c->d_selscr.p;
    B.max_mmp_ext = o->max_mmp_extension > 0 ? o->max_mmp_extension : 7;
    const float cs = (float)o->consensus_slack;        // MappingOpts::consensusSlack is a float (RapMapSAMapper.cpp:138,184-185)
    B.consensus_fraction = cs < 0 ? -cs : ((cs == 0.0) ? 1.0 : (1.0 - cs));   // negative: MappingConfig::consensusFraction itself (qmap_mi355.h)
  }
}

// The first launch: one per chunk behind its own upload (ChunkFeeder), or the whole resident batch as the one chunk.  A launch sees its chunk through
// shifted pointers (offsets are absolute, the per-read / per-unit arrays start at the chunk), the bump allocators, the counters and the status word are shared.
static int launch_first(qm_ctx* c, const StagePlan& p, const RunReq& rq, const DevIndex& ix, const ReadBatch& B, ChunkFeeder* feeder) {
  int rc;
  const int64_t chunk = feeder ? feeder->chunk : p.n;
  for (int64_t u0 = 0; u0 < p.n; u0 += chunk) {
    const int64_t u1 = u0 + chunk < p.n ? u0 + chunk : p.n;
    if (feeder) {
      if ((rc = feeder->upload(feeder->self, u0, u1))) return rc;
      HIPCHK(hipEventRecord(c->evCopy, c->copyStream));
      HIPCHK(hipStreamWaitEvent(c->stream, c->evCopy, 0));
    }
    ReadBatch C = B;
    const int64_t r0 = p.paired ? 2 * u0 : u0, r1 = p.paired ? 2 * u1 : u1;
    C.off1 = B.off1 + u0; if (p.paired) C.off2 = B.off2 + u0;
    C.nreads = r1 - r0; C.lcnt = B.lcnt + r0; C.loff = B.loff + r0;
    if (C.iv_cnt) { C.iv_cnt = B.iv_cnt + r0; C.iv_off = B.iv_off + r0; }
    if (C.found_out) C.found_out = B.found_out + r0;
    if (C.pair_cnt) C.pair_cnt = B.pair_cnt + u0;
    C.read_base = r0;                                 // (what the launch calls read 0: for the skip list)
    const int g = feeder ? map_grid(r1 - r0, c->numCU, p.phc) : p.grid;
    if (p.first == SK_DUO) HIPCHK(qmk_launch_duo(ix, C, c->numCU, c->stream));
    else if (p.first == SK_LEAN || p.first == SK_LEAN_SEL) HIPCHK(qmk_launch_lean(ix, C, c->numCU, c->stream));
    else if (p.first == SK_H2M) HIPCHK(qmk_h2m(ix, C, g, c->numCU, c->stream));
    else HIPCHK(qmk_map_reads(ix, C, p.ns, p.twoPass ? RL_CHAIN_COLLECT : rq.mode == QM_RUN_COLLECT ? RL_ENTRY_COLLECT : RL_FUSED, g, c->numCU, c->stream));
  }
  return QM_OK;
}

// The status word of the scalar block.  1: the list allocator ran out, 16: the interval allocator did (both: grow and redo the batch);
// 2: an SA-interval list beyond QM_GCAP, 4: a read beyond the longest any kernel takes (both: the call fails).  A batch with one of the
// four is redone or refused as a whole (stage_verdict), so no follow-up pass runs over it.  (8, 64: internal errors, reported there too.)
static bool stage_ok(const u64* hscal) { return !(hscal[QM_SC_STATUS] & (1 | 2 | 4 | 16)); }
// The scalar block as everything queued so far leaves it: the host round trip of stage A.  timedMs: the pass recorded evP0 .. evP1 around
// its launch, and that span is added to the call's kernel time (for the N-aware pass also where it runs inside the call's ev0 .. ev1, as ever).
static int read_scalars(qm_ctx* c, u64* hscal, float* timedMs = nullptr) {
  HIPCHK(hipMemcpyAsync(hscal, c->d_scal, QM_SC_WORDS * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  float t = 0; if (timedMs && hipEventElapsedTime(&t, c->evP0, c->evP1) == hipSuccess) *timedMs += t;
  return QM_OK;
}

// The reads of the batch whose lcnt word is `mark` (QM_LCNT_LEAN, QM_LCNT_SLOW), gathered into d_slowq; Q: B pointed at that queue.  nq is the kernels' own count of
// such reads (a scalar slot): the queue is sized for it and the gather writes no more, whatever lcnt holds.  QM_SC_SLOWQ is the gather's cursor; nothing else reads it.
static int gather_queue(qm_ctx* c, unsigned mark, int64_t nq, const ReadBatch& B, ReadBatch& Q) {
  int rc;
  if ((rc = c->d_slowq.ensure(nq))) return rc;
  HIPCHK(hipMemsetAsync(c->d_scal + QM_SC_SLOWQ, 0, sizeof(u64), c->stream));
  HIPCHK(qmk_collect_marked(c->d_lcnt, B.nreads, mark, c->d_slowq, nq, (unsigned long long*)(c->d_scal + QM_SC_SLOWQ), c->stream));
  Q = B; Q.slowq = c->d_slowq; Q.nreads = nq;
  return QM_OK;
}

// The N-aware pass (round 6).  The first-pass kernels leave every read with a character outside A C G T; when many of a batch's reads are
// there for that reason (sequencers write N where a base call failed), qm_lean_kernel's N-aware edition goes over the queue of what was
// left before the general kernel does: reads whose odd characters are all N are mapped at its rate (lean_iter<..., NQ>: k-mers with an N
// are stepped over, MMPs end at one), the others are marked again and counted anew.  hscal: the scalars after the first pass -> after this one.
static int pass_n_aware(qm_ctx* c, const StagePlan& p, const DevIndex& ix, const ReadBatch& B, u64* hscal, float& extraMs) {
  const char* npe = getenv("QM_NPASS_MIN");                      // (read per call: tests switch it; negative: never)
  const long long minDirty = npe ? atoll(npe) : 2048LL;
  if (p.leanWide || minDirty < 0 || p.nreads <= 0) return QM_OK;
#ifndef QM_TIMING
  const int64_t nq = (int64_t)hscal[QM_SC_LEANQ], dirtyReads = (int64_t)hscal[QM_SC_DEFER0];
#else
  const int64_t nq = (int64_t)hscal[QM_SC_LEANQ], dirtyReads = nq;   // (the phase sums sit in the slots of the four reasons, QM_SC_DEFER0 ..)
#endif
  if (nq <= 0 || dirtyReads < minDirty || !stage_ok(hscal)) return QM_OK;
  int rc; ReadBatch Q;
  if ((rc = gather_queue(c, QM_LCNT_LEAN, nq, B, Q))) return rc;
  HIPCHK(hipMemsetAsync(c->d_scal + QM_SC_LEANQ, 0, sizeof(u64), c->stream));
#ifndef QM_TIMING
  HIPCHK(hipMemsetAsync(c->d_scal + QM_SC_DEFER0, 0, 4 * sizeof(u64), c->stream));
#endif
  HIPCHK(hipEventRecord(c->evP0, c->stream));
  HIPCHK(qmk_launch_lean_nq(ix, Q, c->numCU, c->stream));
  HIPCHK(hipEventRecord(c->evP1, c->stream));
  if ((rc = read_scalars(c, hscal, &extraMs))) return rc;
  c->stats.nPass = nq - (int64_t)hscal[QM_SC_LEANQ];
  return QM_OK;
}

// What a lean kernel marked instead of taking (a character that is not A C G T, a long run of one base, a read beyond 128 characters, a
// wide interval, hits on both strands ...): gathered into a queue and taken by the general kernel that does the same job; everything it
// writes goes where the first launch would have put it, and the reads it sets aside in turn (beyond its slot class) take the long-read pass.
static int pass_lean_leftovers(qm_ctx* c, const StagePlan& p, const DevIndex& ix, const ReadBatch& B, u64* hscal, float& extraMs) {
#ifndef QM_TIMING
  for (int i = 0; i < 4; ++i) c->stats.defer[i] = (int64_t)hscal[QM_SC_DEFER0 + i];   // why they were left, as the N-aware pass has it now
#endif
  if (p.duoMerge) c->stats.duoMerged = (int64_t)hscal[4];        // (numReads so far: the pairs the pair kernel merged; stage B's count pass adds the others)
  const int64_t nq = (int64_t)hscal[QM_SC_LEANQ];
  if (nq <= 0 || !stage_ok(hscal)) return QM_OK;
  int rc; ReadBatch Q;
  if ((rc = gather_queue(c, QM_LCNT_LEAN, nq, B, Q))) return rc;
  c->stats.leanDeferred = nq;
  if (p.first == SK_LEAN_SEL) {
    // -s: the general chain-scoring collector, before the list kernels go over all reads and inside the call's ev0 .. ev1; its scalars come
    // down with theirs.  It borrows the scratch reserved for the first launch (p.grid blocks), so it stays within that grid.
    const int g2 = map_grid(nq, c->numCU, p.phc);
    HIPCHK(qmk_map_reads(ix, Q, p.ns, RL_CHAIN_COLLECT, g2 < p.grid ? g2 : p.grid, c->numCU, c->stream));
    return QM_OK;
  }
  // the default call: the general kernels' scratch does not exist yet (B was filled in without it) and is reserved for this launch's own
  // grid -- the dense table's, on the compact -p image too.  The launch comes after ev1: timed by itself.
  const int g2 = map_grid(nq, c->numCU, false);
  if ((rc = gscr_for(c, g2, Q.gslots, Q.ngslots))) return rc;
  Q.gscratch = c->d_gscr;
  HIPCHK(hipEventRecord(c->evP0, c->stream));
  HIPCHK(qmk_map_reads(ix, Q, p.ns, RL_FUSED, g2, c->numCU, c->stream));
  HIPCHK(hipEventRecord(c->evP1, c->stream));
  return read_scalars(c, hscal, &extraMs);
}

// Reads longer than the slot class of the first launch (always: longer than QM_MAX_READ_LEN) were set aside (map_read): gathered and
// mapped by the 32-slot kernels (what: RL_LONG, or RL_LONG_COLLECT for their collector alone) -- a second, small launch; everything it writes (lists, intervals,
// foundHit) goes where the first pass would have put it.
static int pass_long_reads(qm_ctx* c, const StagePlan& p, const DevIndex& ix, const ReadBatch& B, u64* hscal, ReadLaunch what) {
  const int64_t nl = (int64_t)hscal[QM_SC_SLOWCNT];
  if (nl <= 0 || !stage_ok(hscal)) return QM_OK;
  int rc; ReadBatch Q;
  if ((rc = gather_queue(c, QM_LCNT_SLOW, nl, B, Q))) return rc;
  c->stats.slowReads = nl;
  // the launch uses the scratch of the first one, so it stays within its grid; after a lean kernel, which has none, the scratch is reserved here
  const int g2 = map_grid(nl, c->numCU, p.phc), g = g2 < p.grid ? g2 : p.grid;
  if (lean_first(p)) { if ((rc = gscr_for(c, g, Q.gslots, Q.ngslots))) return rc; Q.gscratch = c->d_gscr; }
  HIPCHK(qmk_map_reads(ix, Q, p.ns, what, g, c->numCU, c->stream));
  if (!p.twoPass) return read_scalars(c, hscal);
  // fused -s: the list kernels run next; their own slow queue (reads whose intervals overflow their scratch: pass_sel_slow) starts from zero
  static_assert(QM_SC_SLOWMAX == QM_SC_SLOWCNT + 1, "the queue's count and its largest entry: one memset");
  HIPCHK(hipMemsetAsync(c->d_scal + QM_SC_SLOWCNT, 0, 2 * sizeof(u64), c->stream));
  return QM_OK;
}

// The list kernels of a fused -s call over H, the collectors' intervals.
static int run_list_kernels(qm_ctx* c, const StagePlan& p, const RunReq& rq, const DevIndex& ix, const ReadBatch& H) {
  if (!p.twoPass || p.nreads <= 0) return QM_OK;
  const char* pe = getenv("QM_SEL_PACK");              // 0: the one-read-per-wavefront list kernel for every read (A/B timing, tests)
  if (pe && atoi(pe) == 0) { HIPCHK(qmk_h2m(ix, H, p.grid, c->numCU, c->stream)); return QM_OK; }
  int rc;
  // several reads per wavefront first (qm_selpack.inl); what that kernel cannot take -- hits on both strands, more than 64
  // intervals or suffixes -- it queues, and the one-read-per-wavefront kernel runs over the queue (its length stays on the device)
  if ((rc = c->d_todoq.ensure(p.nreads))) return rc;
  // ... then the wide edition (256 lanes' worth per batch: reads of 150 bp and more) over that queue, which leaves one of its own.
  // A batch of reads beyond 192 characters goes to the wide edition directly: hardly any of them fits the narrow one's 64 lanes
  if ((rc = c->d_todoq2.ensure(p.nreads))) return rc;
  static const int wideFrom = [] { const char* e = getenv("QM_SEL_WIDE_FROM"); return e ? atoi(e) : 192; }();   // (tuning knob)
  if (rq.shortLen > wideFrom) HIPCHK(qmk_h2m_packw(ix, H, nullptr, nullptr, c->d_todoq2, p.grid, c->numCU, c->stream));
  else {
    HIPCHK(qmk_h2m_pack(ix, H, c->d_todoq, p.grid, c->numCU, c->stream));
    HIPCHK(qmk_h2m_packw(ix, H, c->d_todoq, (const unsigned long long*)(c->d_scal + QM_SC_TODO), c->d_todoq2, p.grid, c->numCU, c->stream));
  }
  ReadBatch T = H; T.slowq = c->d_todoq2; T.nreads_dev = c->d_scal + QM_SC_TODO2;
  HIPCHK(qmk_h2m(ix, T, p.grid, c->numCU, c->stream));
  return QM_OK;
}

// -s: reads whose SA intervals hold more suffixes than a wave's scratch (repeats, low-complexity reads) were left on the slow queue: gathered, a few waves given
// scratch sized for the largest, and mapped by the one-read-per-wavefront list kernel (qmk_h2m: what the first launch of a QM_RUN_FROM_INTERVALS call runs too) over its view H
static int pass_sel_slow(qm_ctx* c, const qm_opts* o, const RunReq& rq, const DevIndex& ix, const ReadBatch& H, u64* hscal) {
  if (!o->sel_aln || rq.mode == QM_RUN_COLLECT) return QM_OK;
  const int64_t ns_ = (int64_t)hscal[QM_SC_SLOWCNT];
  if (ns_ <= 0 || !stage_ok(hscal)) return QM_OK;
  int rc; ReadBatch Q;
  const int64_t need = (((int64_t)hscal[QM_SC_SLOWMAX] + 63) / 64) * 64 + 64;
  if ((rc = gather_queue(c, QM_LCNT_SLOW, ns_, H, Q))) return rc;
  const unsigned long long per = (SelScratchDyn::bytes_for(need) + 255) & ~255ULL;
  int64_t waves = ns_ < 256 ? ns_ : 256;
  while (waves > 4 && (unsigned long long)waves * per > (8ULL << 30)) waves /= 2;      // at most 8 GB of scratch
  const int sgrid = (int)((waves + 3) / 4);
  if ((rc = c->d_dynmem.ensure((int64_t)((unsigned long long)sgrid * 4 * per)))) return rc;
  std::vector<SelScratchDyn> hd((size_t)sgrid * 4);       // host image of every wave's struct over its share of the device memory
  for (int w = 0; w < sgrid * 4; ++w) hd[w].bind(c->d_dynmem + (unsigned long long)w * per, need);
  if ((rc = c->d_dyn.ensure((int64_t)(hd.size() * sizeof(SelScratchDyn))))) return rc;
  HIPCHK(hipMemcpyAsync(c->d_dyn, hd.data(), hd.size() * sizeof(SelScratchDyn), hipMemcpyHostToDevice, c->stream));
  Q.dyn = (SelScratchDyn*)c->d_dyn.p; Q.iv_out = nullptr; Q.found_out = nullptr;   // (intervals and foundHit: already written by the first pass)
  HIPCHK(qmk_h2m(ix, Q, sgrid, c->numCU, c->stream));
  if ((rc = read_scalars(c, hscal))) return rc;           // (hd is a local: the copy above is done)
  c->stats.slowReads = ns_;
  return QM_OK;
}

// What the final status word means for the call: QM_OK, an error, or QM_STAGE_RETRY after a bump allocator ran out and its buffer was grown.
enum { QM_STAGE_RETRY = 1 };
static int stage_verdict(qm_ctx* c, const StagePlan& p, const u64* hscal) {
  const int status = (int)(hscal[QM_SC_STATUS] & 0xffffffffu); int rc;
  if (status & 4) return fail(QM_E_TOOLONG, "a read is longer than %d characters (-s: the alignment kernels are sized for that; otherwise the long-read pass takes up to %d)", QM_MAX_LONG_READ_LEN, QM_MAX_LONG_READ_LEN);
  if (status & 2) return fail(QM_E_UNSUPPORTED, "an SA-interval list exceeded %d entries (max_interval too large)", QM_GCAP);
  if (status & 8) return fail(QM_E_STATE, "selective alignment: a read overflowed the scratch sized for it (internal error)");
  if (status & 64) return fail(QM_E_STATE, "a wavefront found no free scratch slot on its XCD (internal error)");
  if (!(status & 17)) return QM_OK;
  if (status & 1) {
    int64_t want = (int64_t)hscal[0] + p.nreads + (int64_t)p.grid * 4 * QM_CHUNK;
    if (want < c->d_lists.cap * 2) want = c->d_lists.cap * 2;
    if ((rc = c->d_lists.ensure(want))) return rc;
  }
  if (status & 16) {
    int64_t want = (int64_t)hscal[QM_SC_IVCUR] + p.nreads + (int64_t)p.grid * 4 * QM_IVCHUNK;
    if (want < c->d_iv.cap * 2) want = c->d_iv.cap * 2;
    if ((rc = c->d_iv.ensure(want))) return rc;
  }
  c->stats.relaunches += 1;
  return QM_STAGE_RETRY;
}

static int run_stage_a(qm_ctx* c, const qm_opts* o, const RunReq& rq, int64_t n, const void* d_seq1, const void* d_off1, const void* d_seq2,
                       const void* d_off2, int ns, ChunkFeeder* feeder, u64* hscal) {
  int rc; StagePlan p;
  if ((rc = plan_stage_a(c, o, rq, d_seq2 != nullptr, n, ns, p))) return rc;
  if ((rc = reserve_stage_a(c, o, rq, p))) return rc;
  const DevIndex ix = dev_index(c);
  const int64_t nreads = p.nreads;
  if (lean_first(p)) c->stats.leanReads = nreads;
  if (p.first == SK_DUO) c->stats.duoPairs = n;
  float extraMs = 0;                                     // the passes timed by themselves (read_scalars' timedMs), over all retries
  while (true) {
    ReadBatch B;
    fill_batch(c, o, rq, p, d_seq1, d_off1, d_seq2, d_off2, B);
    // the list kernels' view of a two-pass -s call (also the slow pass's): the collectors' intervals in (they stay valid, kept for the caller or not), nothing of theirs out
    ReadBatch H = B;
    if (p.twoPass) { H.iv_in = c->d_iv; H.iv_in_off = c->d_ivoff; H.iv_in_cnt = c->d_ivcnt; H.found_in = c->d_found; H.iv_out = nullptr; H.found_out = nullptr; }
    HIPCHK(hipMemsetAsync(c->d_scal, 0, QM_SC_WORDS * sizeof(u64), c->stream));
    if (rq.mode == QM_RUN_COLLECT || p.twoPass) HIPCHK(hipMemsetAsync(c->d_lcnt, 0, (size_t)(nreads + 1) * sizeof(uint32_t), c->stream));   // collector-only kernels write no list lengths: the array only carries the long-read marks
    HIPCHK(hipEventRecord(c->ev0, c->stream));
    if ((rc = launch_first(c, p, rq, ix, B, feeder))) return rc;
    feeder = nullptr;                                     // a retry finds everything resident
    if (p.first == SK_LEAN_SEL && nreads > 0) {          // -s: what the lean collector left reaches the general one before the list kernels run
      if ((rc = read_scalars(c, hscal)) || (rc = pass_n_aware(c, p, ix, B, hscal, extraMs)) || (rc = pass_lean_leftovers(c, p, ix, B, hscal, extraMs))) return rc;
      c->stats.leanReads = nreads;
    }
    // fused -s with reads beyond QM_MAX_READ_LEN in the batch: the counts come down once more, so that the 32-slot collector has their intervals ready for the list kernels
    if (p.twoPass && rq.longReads && nreads > 0 && ((rc = read_scalars(c, hscal)) || (rc = pass_long_reads(c, p, ix, B, hscal, RL_LONG_COLLECT)))) return rc;
    if ((rc = run_list_kernels(c, p, rq, ix, H))) return rc;
    HIPCHK(hipEventRecord(c->ev1, c->stream));
    if ((rc = read_scalars(c, hscal))) return rc;
    if (lean_first(p) && ((rc = pass_n_aware(c, p, ix, B, hscal, extraMs)) || (rc = pass_lean_leftovers(c, p, ix, B, hscal, extraMs)))) return rc;
    if ((!o->sel_aln || rq.mode == QM_RUN_COLLECT) && rq.mode != QM_RUN_FROM_INTERVALS && (rc = pass_long_reads(c, p, ix, B, hscal, rq.mode == QM_RUN_COLLECT ? RL_LONG_COLLECT : RL_LONG))) return rc;
    if ((rc = pass_sel_slow(c, o, rq, ix, H, hscal))) return rc;
#ifdef QM_TIMING
    {                                                    // the phase sums of the -DQM_TIMING kernels: stage A's, qm_h2m_kernel's, the packed list kernels'
      static const char* nm[7] = {"read->LDS", "strand setup", "probe windows", "extension", "collector rest", "hits->mappings", "write-out+loop"};
      double tot = 0; for (int i = 0; i < 7; ++i) tot += (double)hscal[20 + i];
      for (int i = 0; i < 7; ++i) fprintf(stderr, "[qm timing] %-16s %6.2f %%  %10.0f clk/read\n", nm[i], 100.0 * hscal[20 + i] / tot, (double)hscal[20 + i] / (double)nreads);
      static const char* hm[8] = {"intervals in", "suffix gather", "sort", "groups+chain", "list assembly", "(after)", "write-out", "-"};
      double ht = 0; for (int i = 0; i < 8; ++i) ht += (double)hscal[32 + i];
      if (ht > 0) for (int i = 0; i < 8; ++i) fprintf(stderr, "[qm timing h2m] %-16s %6.2f %%  %10.0f clk/read\n", hm[i], 100.0 * hscal[32 + i] / ht, (double)hscal[32 + i] / (double)nreads);
      static const char* pm[8] = {"cand+intervals", "gather+keys", "rank sort", "heads+count", "chaining", "words", "write-out", "chaining, parallel"};
      double pt = 0; for (int i = 0; i < 8; ++i) pt += (double)hscal[40 + i];
      if (pt > 0) for (int i = 0; i < 8; ++i) fprintf(stderr, "[qm timing pack] %-16s %6.2f %%  %10.0f clk/read\n", pm[i], 100.0 * hscal[40 + i] / pt, (double)hscal[40 + i] / (double)nreads);
    }
#endif
    if ((rc = stage_verdict(c, p, hscal)) == QM_STAGE_RETRY) continue;
    if (rc) return rc;
    break;
  }
  // reads that were skipped, not mapped (beyond QM_MAX_LONG_READ_LEN characters; interval lists beyond the scratch): their list
  c->stats.skipped = (int64_t)hscal[QM_SC_SKIPCNT];
  if (c->stats.skipped > 0) {
    c->stats.skipList.resize((size_t)(c->stats.skipped < QM_SKIP_CAP ? c->stats.skipped : QM_SKIP_CAP));
    HIPCHK(hipMemcpy(c->stats.skipList.data(), c->d_skip, c->stats.skipList.size() * sizeof(u64), hipMemcpyDeviceToHost));
  }
  if (p.wantIv) { c->last.ivTotal = (int64_t)hscal[QM_SC_IVCUR]; c->last.ivReads = nreads; }
  if (p.wantFound) c->last.foundReads = nreads;
  if (rq.mode != QM_RUN_COLLECT && !p.duoMerge) c->last.listReads = nreads;   // (pairs the pair kernel merged have no per-read lists)
  c->last.listWords = (int64_t)hscal[0];
  float ms = 0; hipEventElapsedTime(&ms, c->ev0, c->ev1); c->last.mapMs = ms + extraMs;
  return QM_OK;
}

// the temporary storage of the device scans (qmk_scan_counts) over `items` counts
static int ensure_scan_tmp(qm_ctx* c, int64_t items) {
  const size_t stb = qmk_scan_temp_bytes(items);
  return c->d_scanTmp.ensure((int64_t)(stb ? stb : 16));
}

// ---- stage B (+ C with -s): the per-read lists in d_lists -> the units' hits in CSR order.  One thread per unit: count -> scan -> write.
static int run_stage_b(qm_ctx* c, const qm_opts* o, const RunReq& rq, int64_t n, bool paired, const void* d_seq1, const void* d_off1,
                       const void* d_seq2, const void* d_off2, u64* hscal, long long& total) {
  int rc;
  if ((rc = c->d_cnt.ensure(n + 1))) return rc;
  if ((rc = c->d_offs.ensure(n + 1))) return rc;
  if ((rc = ensure_scan_tmp(c, n + 1))) return rc;
  PairBatch P; memset(&P, 0, sizeof(P));
  P.n = n; P.paired = paired ? 1 : 0; P.off1 = (const long long*)d_off1; P.off2 = (const long long*)d_off2;
  P.lcnt = c->d_lcnt; P.loff = c->d_loff; P.lists = c->d_lists; P.cnt = c->d_cnt; P.offs = c->d_offs;
  P.counters = c->d_scal + 1; P.max_num_hits = o->max_num_hits; P.no_orphans = rq.mergeOnly ? 0 : o->no_orphans;
  P.no_dovetail = rq.mergeOnly ? 0 : o->no_dovetail; P.fuzzy = o->fuzzy; P.merge_only = rq.mergeOnly ? 1 : 0;
  if (rq.mergeOnly) {
    if ((rc = c->d_tooMany.ensure(n + 1))) return rc;
    HIPCHK(hipMemsetAsync(c->d_tooMany, 0, (size_t)(n + 1), c->stream));
    P.too_many = c->d_tooMany;
  }
  if (rq.mergeOnly) c->last.tooManyUnits = n;
  HIPCHK(hipMemsetAsync(c->d_cnt + n, 0, sizeof(uint32_t), c->stream));
  if (o->sel_aln) {
    // -s: merge + selective alignment + filter per unit into temp slots, then compaction (qm_sel.inl)
    HIPCHK(qmk_sel_slots(P, c->stream));
    HIPCHK(qmk_scan_counts(c->d_scanTmp, (size_t)c->d_scanTmp.cap, c->d_cnt, c->d_offs, n + 1, 0, c->stream));
    if ((rc = c->d_toff.ensure(n + 1))) return rc;
    HIPCHK(hipMemcpyAsync(c->d_toff, c->d_offs, (size_t)(n + 1) * 8, hipMemcpyDeviceToDevice, c->stream));
    long long slots = 0;
    HIPCHK(hipMemcpyAsync(&slots, c->d_offs + n, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    // chunks of units for plan -> ksw2 -> finish, and where each chunk's slots start (its share of the task buffer)
    const char* cuEnv = getenv("QM_SEL_CHUNK_UNITS");        // (tests: chunk small batches too)
    const int64_t minChunk = cuEnv && atoll(cuEnv) > 0 ? atoll(cuEnv) : 65536;
    const int K = n >= (int64_t)QM_SEL_CHUNKS_B * minChunk ? QM_SEL_CHUNKS_B : 1;
    long long cu[QM_SEL_CHUNKS_B + 1], cslot[QM_SEL_CHUNKS_B + 1];
    for (int i = 0; i <= K; ++i) { cu[i] = n * i / K; cslot[i] = 0; }
    for (int i = 1; i < K; ++i) HIPCHK(hipMemcpyAsync(&cslot[i], c->d_offs + cu[i], sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    cslot[K] = slots;
    if ((rc = c->d_tmp.ensure(slots + 1))) return rc;
    if ((rc = c->d_tsc.ensure(2 * slots + 2))) return rc;
    SelBatch A; memset(&A, 0, sizeof(A));
    A.seq1 = (const unsigned char*)d_seq1; A.seq2 = (const unsigned char*)d_seq2; A.text = c->rep->text;
    A.txp_off = c->rep->txpOff; A.txp_len = c->rep->txpLen; A.tmp = c->d_tmp; A.toff = c->d_toff; A.tsc = c->d_tsc;
    A.match = o->match_score; A.mismatch = o->mismatch_penalty; A.gap_open = o->gap_open; A.gap_extend = o->gap_extend;
    A.long_reads = rq.longReads ? 1 : 0;
    if (rq.longReads && !rq.mergeOnly && sel_ksw_ring_slots(o->dp_bandwidth) > 128) {
      // reads beyond QM_MAX_READ_LEN under a band beyond 97: the alignment blocks of that (slow, rare) edition live in device memory
      if ((rc = c->d_kswRows.ensure((int64_t)qmk_sel_gmem_rows_bytes(c->numCU)))) return rc;
      A.ksw_rows = c->d_kswRows;
    }
    A.short_len = rq.shortLen;
    A.bandwidth = o->dp_bandwidth; A.hard_filter = o->hard_filter; A.policy = o->aln_policy; A.min_score_fraction = o->min_score_fraction;
    { static const int noDiag = [] { const char* e = getenv("QM_SEL_NO_DIAG"); return e ? atoi(e) : 0; }(); A.no_diag = noDiag; }
    HIPCHK(hipMemsetAsync(c->d_cnt + n, 0, sizeof(uint32_t), c->stream));
    if (rq.mergeOnly) {
      HIPCHK(qmk_sel_merge(P, A, c->stream));            // the merge alone: no alignment, chain statuses stay in aln_score
    } else {
      // plan (per unit) -> ksw2 extension alignments, four per wavefront, any band -> finish (per unit)
      if ((rc = c->d_tref.ensure(2 * slots + 2))) return rc;
      if ((rc = c->d_tasks.ensure((2 * slots + 2 * K + 2) * (int64_t)sizeof(SelTask)))) return rc;
      if ((rc = c->d_sides.ensure((2 * slots + 2 * K + 2) * (int64_t)sizeof(SelSide)))) return rc;
      if ((rc = c->d_torder.ensure(2 * (2 * slots + 2 * K + 2)))) return rc;      // (two order lists per chunk: ksw2, strip)
      static const bool noStrip = [] { const char* e = getenv("QM_SEL_NO_STRIP"); return e && atoi(e) != 0; }();
      A.tref = c->d_tref;
      HIPCHK(hipMemsetAsync(c->d_ntk, 0, 3 * QM_SEL_CHUNKS_B * sizeof(u64), c->stream));
      // The plan (three kernels: per unit, per alignment question, per question) waits on scattered loads and the ksw2 kernel is
      // bound by VALU issue: the plans of chunks 1.. run on a stream of their own while the alignments of the chunks before
      // them are computed.
      HIPCHK(hipEventRecord(c->evPlan[QM_SEL_CHUNKS_B], c->stream));
      HIPCHK(hipStreamWaitEvent(c->planStream, c->evPlan[QM_SEL_CHUNKS_B], 0));
      SelBatch Ak[QM_SEL_CHUNKS_B];
      static const bool serial = [] { const char* e = getenv("QM_SEL_SERIAL"); return e && atoi(e) != 0; }();   // (profiling: no plan stream, every kernel's duration is its own)
      hipStream_t planStream = K > 1 && !serial ? c->planStream : c->stream;
      for (int i = 0; i < K; ++i) {
        Ak[i] = A; Ak[i].u0 = cu[i]; Ak[i].u1 = cu[i + 1];
        Ak[i].tasks = (SelTask*)(c->d_tasks + (size_t)(2 * cslot[i] + 2 * i) * sizeof(SelTask));   // at most two tasks per slot
        Ak[i].ntasks = c->d_ntk + i;
        Ak[i].sides = (SelSide*)(c->d_sides + (size_t)(2 * cslot[i] + 2 * i) * sizeof(SelSide));       // ... and at most two questions
        Ak[i].nsides = c->d_ntk + QM_SEL_CHUNKS_B + i;
        Ak[i].torder = c->d_torder + (size_t)(2 * cslot[i] + 2 * i);
        if (!noStrip) { Ak[i].torder2 = c->d_torder + (size_t)(2 * slots + 2 * K + 2) + (size_t)(2 * cslot[i] + 2 * i); Ak[i].ntasks2 = c->d_ntk + 2 * QM_SEL_CHUNKS_B + i; }
        HIPCHK(qmk_sel_plan(P, Ak[i], c->numCU, planStream));
        if (K > 1) HIPCHK(hipEventRecord(c->evPlan[i], planStream));
      }
      for (int i = 0; i < K; ++i) {
        if (K > 1) HIPCHK(hipStreamWaitEvent(c->stream, c->evPlan[i], 0));
        HIPCHK(qmk_sel_align_finish(P, Ak[i], c->numCU, c->stream));
      }
    }
  } else {
    HIPCHK(qmk_pair_count(P, c->stream));
  }
  // one part of a split call: the scan starts from the hits of the parts before this one and writes straight into the caller's offsets
  // (entry n, the closing one, is also the first entry of the part behind this one, which writes the same number there)
  long long base = 0; long long* offsOut = c->d_offs;
  if (rq.join) {
    if ((rc = rq.join->wait_base(rq.part, base))) return rc;
    offsOut = rq.join->owner->d_offs + rq.u0;
  }
  HIPCHK(qmk_scan_counts(c->d_scanTmp, (size_t)c->d_scanTmp.cap, c->d_cnt, offsOut, n + 1, base, c->stream));
  total = 0;
  HIPCHK(hipMemcpyAsync(&total, offsOut + n, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(hscal, c->d_scal, QM_SC_WORDS * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  u64 h[3 * QM_SEL_CHUNKS_B];
  const bool selStats = o->sel_aln && !rq.mergeOnly;
  if (selStats) HIPCHK(hipMemcpyAsync(h, c->d_ntk, sizeof(h), hipMemcpyDeviceToHost, c->stream));   // (with the synchronisation that follows anyway)
  HIPCHK(hipStreamSynchronize(c->stream));
  if (selStats) {
    for (int i = 0; i < QM_SEL_CHUNKS_B; ++i) { c->stats.kswTasks += (int64_t)h[i]; c->stats.selQuestions += (int64_t)h[QM_SEL_CHUNKS_B + i]; c->stats.stripTasks += (int64_t)h[2 * QM_SEL_CHUNKS_B + i]; }
    static const bool dbg = [] { const char* e = getenv("QM_SEL_DEBUG"); return e && atoi(e) != 0; }();
    if (dbg) fprintf(stderr, "[qm -s] %lld units: %lld alignment questions beyond PERFECT chains, %lld ksw2 alignments, %lld strip alignments\n", (long long)n, (long long)c->stats.selQuestions, (long long)c->stats.kswTasks, (long long)c->stats.stripTasks);
  }
  if (rq.join) {
    // the offsets are the caller's own (absolute), so the records go to the caller's array itself; written now if it has the room,
    // and once more if a part behind this one had it replaced (SplitJoin)
    total -= base;
    qm_hit* dst = nullptr; bool early = false, again = false;
    if ((rc = rq.join->place(rq.part, total, dst, early))) return rc;
    P.offs = offsOut;
    for (int pass = 0; pass < 2; ++pass) {
      P.hits = dst;
      if (o->sel_aln) HIPCHK(qmk_sel_compact(P, c->d_tmp, c->d_toff, c->stream));
      else HIPCHK(qmk_pair_write(P, c->stream));
      if (pass) break;
      HIPCHK(hipStreamSynchronize(c->stream));
      if ((rc = rq.join->settle(rq.part, early, again, dst))) return rc;
      if (!again) break;
    }
    return QM_OK;
  }
  if ((rc = c->d_hits.ensure((int64_t)total + 1, total / 8))) return rc;
  P.hits = c->d_hits;
  if (o->sel_aln) HIPCHK(qmk_sel_compact(P, c->d_tmp, c->d_toff, c->stream));
  else HIPCHK(qmk_pair_write(P, c->stream));
  return QM_OK;
}

static int map_device_impl(qm_ctx* c, const qm_opts* o, int64_t n, const void* d_seq1, const void* d_off1, const void* d_seq2,
                           const void* d_off2, int32_t max_read_len, int64_t* n_hits, qm_counters* counters, ChunkFeeder* feeder,
                           const RunReq& rq = RunReq(), int32_t short_read_len = 0) {
  if (!c || n < 0 || (n > 0 && (!d_seq1 || !d_off1))) return fail(QM_E_ARG, "bad argument");
  int rc = check_opts(o);
  if (rc) return rc;
  if ((d_seq2 == nullptr) != (d_off2 == nullptr)) return fail(QM_E_ARG, "seq2/off2 must both be given or both be null");
  // (a read beyond QM_MAX_LONG_READ_LEN is skipped, not mapped: qm_fetch_skipped)
  HIPCHK(hipSetDevice(c->device));
  // 64-character slots per read: picks the kernel instantiation.  `short_read_len` (host callers: the longest read that is not
  // beyond QM_MAX_READ_LEN) picks it when the batch also holds long reads -- those are set aside by the launch whatever its
  // slot class and mapped by the long-read pass
  const int pick = (max_read_len > QM_MAX_READ_LEN && short_read_len > 0) ? short_read_len : (max_read_len > QM_MAX_READ_LEN ? QM_MAX_READ_LEN : max_read_len);
  const int ns = pick <= 128 ? 2 : (pick <= 192 ? 3 : (pick <= 256 ? 4 : 8));
  const bool paired = d_seq2 != nullptr;
  u64 hscal[QM_SC_WORDS];
  begin_call(c);
  HIPCHK(hipEventRecord(c->evA, c->stream));
  RunReq r2 = rq;
  r2.keepIntervals = rq.keepIntervals || c->debug != 0;
  r2.longReads = max_read_len > QM_MAX_READ_LEN;
  r2.shortLen = pick;
  if (rq.join && (rc = rq.join->wait_turn(rq.part))) return rc;
  rc = run_stage_a(c, o, r2, n, d_seq1, d_off1, d_seq2, d_off2, ns, feeder, hscal);
  if (rq.join) rq.join->pass_turn(rq.part);
  if (rc) return rc;
  if (r2.stageView) {
    // where every read's interval records and list words will sit in CSR order: two scans behind stage A; their totals come
    // down with the synchronisation stage B needs anyway
    const int64_t nreads = paired ? 2 * n : n;
    if ((rc = c->d_ivcsr.ensure(nreads + 1))) return rc;
    if ((rc = c->d_lcsr.ensure(nreads + 1))) return rc;
    if ((rc = c->h_tot.ensure(2))) return rc;
    if ((rc = ensure_scan_tmp(c, nreads + 1))) return rc;
    if (!r2.keepIntervals) {
      // a stage view without the SA-interval records (QM_STAGES_NO_INTERVALS): every read's count is zero
      if ((rc = c->d_ivcnt.ensure(nreads + 1))) return rc;
      if ((rc = c->d_ivoff.ensure(nreads + 1))) return rc;
      if ((rc = c->d_iv.ensure(1))) return rc;
      HIPCHK(hipMemsetAsync(c->d_ivcnt, 0, (size_t)(nreads + 1) * sizeof(uint32_t), c->stream));
      HIPCHK(hipMemsetAsync(c->d_ivoff, 0, (size_t)(nreads + 1) * sizeof(long long), c->stream));
    }
    HIPCHK(hipMemsetAsync(c->d_ivcnt + nreads, 0, sizeof(uint32_t), c->stream));
    HIPCHK(hipMemsetAsync(c->d_lcnt + nreads, 0, sizeof(uint32_t), c->stream));
    HIPCHK(qmk_scan_counts(c->d_scanTmp, (size_t)c->d_scanTmp.cap, c->d_ivcnt, c->d_ivcsr, nreads + 1, 0, c->stream));
    HIPCHK(qmk_scan_counts_masked(c->d_scanTmp, (size_t)c->d_scanTmp.cap, c->d_lcnt, c->d_lcsr, nreads + 1, c->stream));
    HIPCHK(hipMemcpyAsync(&c->h_tot[0], c->d_ivcsr + nreads, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&c->h_tot[1], c->d_lcsr + nreads, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    c->last.stReads = nreads;
  }
  long long total = 0;
  if ((rc = run_stage_b(c, o, r2, n, paired, d_seq1, d_off1, d_seq2, d_off2, hscal, total))) return rc;
  HIPCHK(hipEventRecord(c->evB, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  float ms = 0; hipEventElapsedTime(&ms, c->evA, c->evB); c->last.totalMs = ms;
  c->last.units = n; c->last.hits = total; c->last.paired = paired;
  if (r2.stageView) c->last.stUnits = n;
  if (n_hits) *n_hits = total;
  if (counters) *counters = counters_from(hscal);
  return QM_OK;
}

// the hits of the parts before `part`, once all of them have brought their totals (or a part has failed: no total may come)
int SplitJoin::wait_base(int part, long long& b) {
  std::unique_lock<std::mutex> lk(mu);
  cv.wait(lk, [&] { if (failed) return true; for (int i = 0; i < part; ++i) if (!have[i]) return false; return true; });
  if (failed) return failure();
  b = 0;
  for (int i = 0; i < part; ++i) b += total[i];
  return QM_OK;
}

// part `part` has `tot` hits: where may it write them?  early: into the array as it stands, now (counted in `inflight` until settle()).
// Otherwise -- the array is too small for base + tot records, or another part found it so -- the part waits until every total is known
// and no early write is in flight; the first part through sizes the array for the whole batch.
int SplitJoin::place(int part, long long tot, qm_hit*& dst, bool& early) {
  std::unique_lock<std::mutex> lk(mu);
  total[part] = tot; have[part] = true; ++arrived;
  long long b = 0;
  for (int i = 0; i < part; ++i) b += total[i];
  cv.notify_all();
  if (failed) return failure();
  early = !needGrow && owner->d_hits.p && owner->d_hits.cap >= b + tot + 1;
  if (early) { ++inflight; dst = owner->d_hits; return QM_OK; }
  needGrow = true;
  cv.wait(lk, [&] { return failed || (arrived == K && inflight == 0); });
  if (failed) return failure();
  if (!sized) {
    for (int i = 0; i < K; ++i) base[i + 1] = base[i] + total[i];
    const int rc = owner->d_hits.ensure((int64_t)base[K] + 1, base[K] / 8);
    if (rc) { failed = rc; cv.notify_all(); return failure(); }
    sized = true;
    cv.notify_all();
  }
  dst = owner->d_hits;
  return QM_OK;
}

// part `part` has written its hits and synchronised.  again: it wrote early and the array has been replaced since -- write once more, to dst.
// (Whether the array is replaced is known once every part has brought its total.)
int SplitJoin::settle(int part, bool early, bool& again, qm_hit*& dst) {
  std::unique_lock<std::mutex> lk(mu);
  if (early) { --inflight; cv.notify_all(); }
  again = false;
  if (!early) return failed ? failure() : QM_OK;
  cv.wait(lk, [&] { return failed || (arrived == K && (!needGrow || sized)); });
  if (failed) return failure();
  if (needGrow) { again = true; dst = owner->d_hits; }
  return QM_OK;
}

// A large device-resident batch in K parts, each on a helper context of the same replica (own stream, own work buffers),
// in flight together: the tail of one part's persistent stage-A grid, its scans, its host round trips and (with -s) its
// VALU-bound alignment kernels run under the other parts' stage A, which is bound by the scalar unit and by waiting
// (profiles/r04/sel_overlap.txt).  Units, hits and counters are those of one call: part i maps units [n i / K, n (i + 1) / K),
// its hits land in the caller's array behind those of the parts before it and its offsets are the caller's own: a part scans its counts
// from the hits in front of it and depends on the parts before it alone (SplitJoin) -- the part that finishes first should be part 0.
static int map_device_split(qm_ctx* c, const qm_opts* o, int K, int64_t n, const void* d_seq1, const void* d_off1, const void* d_seq2,
                            const void* d_off2, int32_t max_read_len, int64_t* n_hits, qm_counters* counters) {
  int rc;
  HIPCHK(hipSetDevice(c->device));
  while ((int)c->helpers.size() < K) {
    qm_ctx* h = nullptr;
    if ((rc = qm_ctx_create_ex(c->ix, c->device, c->flags, &h))) return rc;
    h->isHelper = true; c->helpers.push_back(h);
  }
  if (!c->pool || (int)c->pool->th.size() < K) { delete c->pool; c->pool = new SplitPool(K); }
  if ((rc = c->d_offs.ensure(n + 1))) return rc;
  SplitJoin J; J.owner = c; J.K = K;
  { const char* sg = getenv("QM_SPLIT_STAGGER"); J.stagger = sg ? atoi(sg) != 0 : false; }   // (measured: 73.6-75.4 against 76.4 M pairs/s with all parts started at once -- the kernels are all bound by instruction issue, whichever unit)
  int64_t nh[8] = {0}; qm_counters ctr[8]; int rcs[8] = {0}; char errs[8][256];
  memset(ctr, 0, sizeof(ctr));
  const bool paired = d_seq2 != nullptr;
  // QM_SPLIT_FIRST: two parts of unequal size -- the share of PART 0 in per cent, which by default is the qm_lean_kernel part (the pair
  // kernel's share is the rest); unset: halves
  static const int firstPct = [] { const char* e = getenv("QM_SPLIT_FIRST"); const int v = e ? atoi(e) : 0; return v > 0 && v < 100 ? v : 0; }();
  auto first_unit = [&](int i) { return (K == 2 && firstPct > 0) ? (i == 0 ? (int64_t)0 : (i == 1 ? n * firstPct / 100 : n)) : n * i / K; };
  // Which parts take the pair kernel (a bit per part; QM_DUO_PARTS): the others take qm_lean_kernel.  The pair kernel is bound by the
  // vector units (919 VALU + 470 scalar-side instructions per pair), qm_lean_kernel by the CU's scalar unit (756 + 1 125): with a part
  // of each kind in flight the two kinds of wavefront share every CU and each loads the unit the other leaves idle -- 492 M pairs/s
  // against 447 (all parts the pair kernel) and 473 (all parts qm_lean_kernel), profiles/r06/exp_mix.txt
  // The default is every other part from part 1 on: part 0 takes qm_lean_kernel, which finishes first (17.8 against 19.7 ms on the headline
  // batch), so its scan, its round trip and its write pass are over before the pair-kernel part behind it needs its total.  Which kernel maps
  // which pairs does not change the hits.
  static const int duoParts = [] { const char* e = getenv("QM_DUO_PARTS"); return e ? atoi(e) : 0xAA; }();
  begin_call(c);
  HIPCHK(hipEventRecord(c->evA, c->stream));
  c->pool->run(K, [&](int i) {
    qm_ctx* h = c->helpers[(size_t)i];
    const int64_t u0 = first_unit(i), u1 = first_unit(i + 1);
    RunReq rq; rq.join = &J; rq.part = i; rq.u0 = u0;
    rq.noDuo = ((duoParts >> i) & 1) == 0;
    errs[i][0] = 0;
    int r = map_device_impl(h, o, u1 - u0, d_seq1, (const long long*)d_off1 + u0, d_seq2, d_seq2 ? (const long long*)d_off2 + u0 : nullptr,
                            max_read_len, &nh[i], &ctr[i], nullptr, rq);
    if (r != QM_OK) { snprintf(errs[i], sizeof(errs[i]), "%s", g_err); J.abort(r); }
    rcs[i] = r;
  });
  for (int i = 0; i < K; ++i) if (rcs[i]) return fail(rcs[i], "%s", errs[i]);
  HIPCHK(hipEventRecord(c->evB, c->stream));
  HIPCHK(hipEventSynchronize(c->evB));
  // stage A's span: first start to last end over the parts (events of different streams of one device compare)
  float first = 1e30f, last = 0, t = 0;
  for (int i = 0; i < K; ++i) {
    qm_ctx* h = c->helpers[(size_t)i];
    if (hipEventElapsedTime(&t, c->evA, h->ev0) == hipSuccess && t < first) first = t;
    if (hipEventElapsedTime(&t, c->evA, h->ev1) == hipSuccess && t > last) last = t;
  }
  c->last.mapMs = last > first ? last - first : 0;
  float ms = 0; hipEventElapsedTime(&ms, c->evA, c->evB); c->last.totalMs = ms;
  qm_counters sum; memset(&sum, 0, sizeof(sum));
  long long hits = 0;
  for (int i = 0; i < K; ++i) {
    sum += ctr[i];
    const int64_t u0 = first_unit(i);
    c->stats.add_part(c->helpers[(size_t)i]->stats, paired ? 2 * u0 : u0);
    hits += J.total[i];
  }
  c->last.units = n; c->last.hits = hits; c->last.paired = paired;
  if (n_hits) *n_hits = hits;
  if (counters) *counters = sum;
  return QM_OK;
}

int qm_map_device(qm_ctx* c, const qm_opts* o, int64_t n, const void* d_seq1, const void* d_off1, const void* d_seq2,
                  const void* d_off2, int32_t max_read_len, int64_t* n_hits, qm_counters* counters) {
  // Two parts in flight together for batches of 2 M units and more (QM_SPLIT: how many; 1: none).  With -s the parts' alignment kernels
  // run under each other's stage A.  Without -s a call was stage A and little else until round 5; behind the lean kernel the pair
  // kernels, scans and synchronisations of stage B are a tenth of the step: with two parts started together (their stage-A launches
  // share the chip, each about as long as one launch over the whole batch) whichever part is ahead runs its stage B under the other's
  // stage A (434.8 -> 456.7 M pairs/s on config 2).
  const char* me = getenv("QM_SPLIT_MIN");                 // (tests: split small batches too)
  const int64_t minUnits = me && atoll(me) > 0 ? atoll(me) : ((int64_t)1 << 21);
  if (c && o && !c->isHelper && !c->debug && n >= minUnits && d_seq1 && d_off1 && (d_seq2 == nullptr) == (d_off2 == nullptr) && check_opts(o) == QM_OK) {
    const char* se = getenv("QM_SPLIT");
    int K = se ? atoi(se) : 2;
    if (K > 8) K = 8;
    if (K > 1) return map_device_split(c, o, K, n, d_seq1, d_off1, d_seq2, d_off2, max_read_len, n_hits, counters);
  }
  return map_device_impl(c, o, n, d_seq1, d_off1, d_seq2, d_off2, max_read_len, n_hits, counters, nullptr);
}

// offsets of one mate: monotone, longest read; device copies of the offsets (copy stream) and room for the characters
static int stage_offsets(qm_ctx* c, int64_t n, const int64_t* off, DevBuf<uint8_t>& d_seq, DevBuf<long long>& d_off, int32_t& maxLen,
                         int32_t& maxShort) {
  for (int64_t i = 0; i < n; ++i) {
    int64_t l = off[i + 1] - off[i];
    if (l < 0) return fail(QM_E_ARG, "offsets not monotone");
    if (l > maxLen) maxLen = (int32_t)(l > 0x7fffffff ? 0x7fffffff : l);
    if (l <= QM_MAX_READ_LEN && l > maxShort) maxShort = (int32_t)l;
  }
  int rc;
  if ((rc = d_seq.ensure(off[n] + 64))) return rc;
  if ((rc = d_off.ensure(n + 1))) return rc;
  HIPCHK(hipMemcpyAsync(d_off, off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, c->copyStream));
  return QM_OK;
}

struct HostFeed { qm_ctx* c; const char* seq1; const int64_t* off1; const char* seq2; const int64_t* off2; };
static int host_feed_upload(void* self, int64_t u0, int64_t u1) {
  HostFeed* f = (HostFeed*)self;
  const int64_t a1 = f->off1[u0], b1 = f->off1[u1];
  // (pageable memory through the runtime's own staging: 35 GB/s on the round's boxes -- eight threads copying into pinned buffers of our own
  // were no faster, profiles/r06/exp_mix.txt)
  if (b1 > a1) HIPCHK(hipMemcpyAsync(f->c->d_seq1 + a1, f->seq1 + a1, (size_t)(b1 - a1), hipMemcpyHostToDevice, f->c->copyStream));
  if (f->seq2) {
    const int64_t a2 = f->off2[u0], b2 = f->off2[u1];
    if (b2 > a2) HIPCHK(hipMemcpyAsync(f->c->d_seq2 + a2, f->seq2 + a2, (size_t)(b2 - a2), hipMemcpyHostToDevice, f->c->copyStream));
  }
  return QM_OK;
}

static int map_host(qm_ctx* c, const qm_opts* o, int64_t n, const char* seq1, const int64_t* off1, const char* seq2,
                    const int64_t* off2, int64_t* n_hits, qm_counters* counters, const RunReq& rq) {
  if (!c || n < 0 || (n > 0 && (!seq1 || !off1))) return fail(QM_E_ARG, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  int32_t maxLen = 0, maxShort = 0; int rc;
  static const int64_t zero = 0;
  if (n == 0) { off1 = &zero; if (seq2) off2 = &zero; }
  if ((rc = check_opts(o))) return rc;
  if ((rc = stage_offsets(c, n, off1, c->d_seq1, c->d_off1, maxLen, maxShort))) return rc;
  if (seq2 && (rc = stage_offsets(c, n, off2, c->d_seq2, c->d_off2, maxLen, maxShort))) return rc;
  // the characters follow chunk by chunk, each chunk's kernel behind its own copy (ChunkFeeder); QM_HOST_CHUNK = units per chunk
  HostFeed hf = {c, seq1, off1, seq2, off2};
  const char* ce = getenv("QM_HOST_CHUNK");
  ChunkFeeder fd; fd.chunk = ce && atoll(ce) > 0 ? atoll(ce) : (1 << 20); fd.upload = host_feed_upload; fd.self = &hf;
  rc = map_device_impl(c, o, n, c->d_seq1, c->d_off1, seq2 ? c->d_seq2 : nullptr, seq2 ? c->d_off2 : nullptr, maxLen, n_hits, counters, &fd, rq, maxShort > 0 ? maxShort : 1);
  hipStreamSynchronize(c->copyStream);                     // nothing of the caller's buffers is in flight after return (error paths too)
  return rc;
}

int qm_map_pairs(qm_ctx* c, const qm_opts* o, int64_t n, const char* seq1, const int64_t* off1, const char* seq2,
                 const int64_t* off2, int64_t* n_hits, qm_counters* counters) {
  if (!seq2 || !off2) return fail(QM_E_ARG, "qm_map_pairs needs both mates");
  return map_host(c, o, n, seq1, off1, seq2, off2, n_hits, counters, RunReq());
}

int qm_map_reads(qm_ctx* c, const qm_opts* o, int64_t n, const char* seq, const int64_t* off, int64_t* n_hits,
                 qm_counters* counters) {
  return map_host(c, o, n, seq, off, nullptr, nullptr, n_hits, counters, RunReq());
}

// 2-bit packed reads in, the ASCII image the kernels read built on the device (include/qmap_mi355.h)
static int unpack_mate(qm_ctx* c, int64_t n, const uint8_t* pk, const int64_t* off, const qm_pack_exc* exc, int64_t nexc, DevBuf<uint8_t>& d_seq,
                       DevBuf<long long>& d_off, DevBuf<uint8_t>& d_pk, DevBuf<qm_pack_exc>& d_exc, int32_t& maxLen, int32_t& maxShort) {
  int32_t mateMax = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t l = off[i + 1] - off[i];
    if (l < 0) return fail(QM_E_ARG, "offsets not monotone");
    if (l > mateMax) mateMax = (int32_t)(l > 0x7fffffff ? 0x7fffffff : l);
    if (l <= QM_MAX_READ_LEN && l > maxShort) maxShort = (int32_t)l;
  }
  if (mateMax > maxLen) maxLen = mateMax;
  if (off[n] > 0xffffffffLL) return fail(QM_E_ARG, "more than 2^32 characters in one packed batch");
  int rc;
  const int64_t pkBytes = qm_packed_bytes(off, n);
  if ((rc = d_seq.ensure(off[n] + 64))) return rc;
  if ((rc = d_off.ensure(n + 1))) return rc;
  if ((rc = d_pk.ensure(pkBytes))) return rc;
  if ((rc = d_exc.ensure(nexc + 1))) return rc;
  HIPCHK(hipMemcpyAsync(d_off, off, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(d_pk, pk, (size_t)pkBytes - 8, hipMemcpyHostToDevice, c->stream));
  if (nexc > 0) HIPCHK(hipMemcpyAsync(d_exc, exc, (size_t)nexc * sizeof(qm_pack_exc), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(d_seq + off[n], 0, 64, c->stream));      // the mapper fetches reads a word at a time: defined bytes behind the last one
  HIPCHK(qmk_unpack_reads(d_pk, d_off, n, off[n], d_seq, d_exc, nexc, c->stream));
  return QM_OK;
}

static int map_packed(qm_ctx* c, const qm_opts* o, int64_t n, const uint8_t* pk1, const int64_t* off1, const qm_pack_exc* exc1, int64_t nexc1,
                      const uint8_t* pk2, const int64_t* off2, const qm_pack_exc* exc2, int64_t nexc2, int64_t* n_hits, qm_counters* counters, const RunReq& rq = RunReq()) {
  if (!c || n < 0 || (n > 0 && (!pk1 || !off1)) || nexc1 < 0 || nexc2 < 0 || (nexc1 > 0 && !exc1) || (nexc2 > 0 && !exc2)) return fail(QM_E_ARG, "bad argument");
  HIPCHK(hipSetDevice(c->device));
  int rc;
  if ((rc = check_opts(o))) return rc;
  static const int64_t zero[2] = {0, 0};
  static const uint8_t none[8] = {0};
  if (n == 0) { off1 = zero; pk1 = none; if (pk2) { off2 = zero; pk2 = none; } }
  int32_t maxLen = 0, maxShort = 0;
  if ((rc = unpack_mate(c, n, pk1, off1, exc1, nexc1, c->d_seq1, c->d_off1, c->d_pk1, c->d_exc1, maxLen, maxShort))) return rc;
  if (pk2 && (rc = unpack_mate(c, n, pk2, off2, exc2, nexc2, c->d_seq2, c->d_off2, c->d_pk2, c->d_exc2, maxLen, maxShort))) return rc;
  rc = map_device_impl(c, o, n, c->d_seq1, c->d_off1, pk2 ? c->d_seq2 : nullptr, pk2 ? c->d_off2 : nullptr, maxLen, n_hits, counters, nullptr, rq, maxShort > 0 ? maxShort : 1);
  hipStreamSynchronize(c->stream);                         // nothing of the caller's buffers is in flight after return (error paths too)
  return rc;
}

int qm_map_pairs_packed(qm_ctx* c, const qm_opts* o, int64_t n, const uint8_t* pk1, const int64_t* off1, const qm_pack_exc* exc1, int64_t nexc1,
                        const uint8_t* pk2, const int64_t* off2, const qm_pack_exc* exc2, int64_t nexc2, int64_t* n_hits, qm_counters* counters) {
  if (!pk2 || !off2) return fail(QM_E_ARG, "qm_map_pairs_packed needs both mates");
  return map_packed(c, o, n, pk1, off1, exc1, nexc1, pk2, off2, exc2, nexc2, n_hits, counters);
}
int qm_map_reads_packed(qm_ctx* c, const qm_opts* o, int64_t n, const uint8_t* pk, const int64_t* off, const qm_pack_exc* exc, int64_t nexc,
                        int64_t* n_hits, qm_counters* counters) {
  return map_packed(c, o, n, pk, off, exc, nexc, nullptr, nullptr, nullptr, 0, n_hits, counters);
}

// device -> the caller's (pageable) memory, one array
static int staged_download(qm_ctx* c, void* dstv, const void* d_src, size_t bytes) {
    if (bytes < ((size_t)64 << 20)) HIPCHK(hipMemcpy(dstv, d_src, bytes, hipMemcpyDeviceToHost));
    else {
      unsigned char* const hits = (unsigned char*)dstv;
      // (a result array the caller has just allocated is a million page faults: ask for huge pages where the range holds whole ones --
      // a hint, honoured where transparent huge pages are on `madvise` or `always`)
      {
        const uintptr_t a = ((uintptr_t)hits + ((uintptr_t)2 << 20) - 1) & ~(((uintptr_t)2 << 20) - 1), e = ((uintptr_t)hits + bytes) & ~(((uintptr_t)2 << 20) - 1);
        static const bool thp = [] { const char* v = getenv("QM_FETCH_THP"); return !(v && atoi(v) == 0); }();
        if (thp && e > a) madvise((void*)a, (size_t)(e - a), MADV_HUGEPAGE);
      }
      // A large result lands in memory the caller has usually just allocated (every page still to be faulted in), where a
      // plain pageable hipMemcpy runs at ~9 GB/s.  Instead: DMA into two pinned staging buffers in turn at PCIe rate while
      // host threads copy the previous chunk into the caller's array, so the page faults are spread over several cores.
      const size_t CH = (size_t)32 << 20;
      if (int rc = c->h_stage.ensure(2 * CH)) return rc;
      if (!c->evStage[0]) { HIPCHK(hipEventCreateWithFlags(&c->evStage[0], hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&c->evStage[1], hipEventDisableTiming)); }
      const size_t nch = (bytes + CH - 1) / CH;
      auto drain = [&](size_t i) -> hipError_t {             // chunk i: staging -> caller's array, 8 threads
        hipError_t e = hipEventSynchronize(c->evStage[i & 1]);
        if (e != hipSuccess) return e;
        const size_t off = i * CH, len = off + CH <= bytes ? CH : bytes - off;
        const unsigned char* src = c->h_stage + (i & 1) * CH; unsigned char* dst = hits + off;
        const int nt = 8; std::vector<std::thread> th;
        const size_t per = ((len + nt - 1) / nt + 4095) & ~(size_t)4095;
        for (int t = 0; t < nt; ++t) {
          const size_t a0 = per * (size_t)t; if (a0 >= len) break;
          const size_t l0 = a0 + per <= len ? per : len - a0;
          th.emplace_back([=]() { memcpy(dst + a0, src + a0, l0); });
        }
        for (auto& x : th) x.join();
        return hipSuccess;
      };
      for (size_t i = 0; i < nch; ++i) {
        const size_t off = i * CH, len = off + CH <= bytes ? CH : bytes - off;
        HIPCHK(hipMemcpyAsync(c->h_stage + (i & 1) * CH, (const unsigned char*)d_src + off, len, hipMemcpyDeviceToHost, c->copyStream));
        HIPCHK(hipEventRecord(c->evStage[i & 1], c->copyStream));
        if (i > 0) HIPCHK(drain(i - 1));
      }
      HIPCHK(drain(nch - 1));
    }
  return QM_OK;
}

int qm_fetch_hits(qm_ctx* c, int64_t* hit_offsets, qm_hit* hits) {
  if (!c || c->last.units < 0) return fail(QM_E_STATE, "no mapping result to fetch");
  HIPCHK(hipSetDevice(c->device));
  int rc;
  if (hit_offsets && (rc = staged_download(c, hit_offsets, c->d_offs, (size_t)(c->last.units + 1) * 8))) return rc;
  if (hits && c->last.hits > 0 && (rc = staged_download(c, hits, c->d_hits, (size_t)c->last.hits * sizeof(qm_hit)))) return rc;
  return QM_OK;
}

int qm_fetch_hits_pinned(qm_ctx* c, int64_t* hit_offsets, qm_hit* hits) {
  if (!c || c->last.units < 0) return fail(QM_E_STATE, "no mapping result to fetch");
  HIPCHK(hipSetDevice(c->device));
  if (hit_offsets) HIPCHK(hipMemcpyAsync(hit_offsets, c->d_offs, (size_t)(c->last.units + 1) * 8, hipMemcpyDeviceToHost, c->copyStream));
  if (hits && c->last.hits > 0) HIPCHK(hipMemcpyAsync(hits, c->d_hits, (size_t)c->last.hits * sizeof(qm_hit), hipMemcpyDeviceToHost, c->copyStream));
  HIPCHK(hipStreamSynchronize(c->copyStream));
  return QM_OK;
}

int qm_result_device(qm_ctx* c, const void** d_hit_offsets, const void** d_hits) {
  if (!c || c->last.units < 0) return fail(QM_E_STATE, "no mapping result");
  if (d_hit_offsets) *d_hit_offsets = c->d_offs;
  if (d_hits) *d_hits = c->d_hits;
  return QM_OK;
}

int qm_fetch_intervals(qm_ctx* c, int64_t* int_offsets, qm_sa_interval_hit* ints, int64_t cap) {
  if (!c || c->last.ivReads < 0) return fail(QM_E_STATE, "no SA-interval hits kept (qm_ctx_set_debug / qm_collect_reads / qm_map_pairs_stages before mapping)");
  if (!int_offsets) return fail(QM_E_ARG, "null int_offsets");
  HIPCHK(hipSetDevice(c->device));
  // per unit: a pair's four lists (left fwd, left rc, right fwd, right rc) follow each other; a single read's two
  const int64_t nreads = c->last.ivReads;
  const int mates = (c->last.units >= 0 && c->last.paired && c->last.ivReads == 2 * c->last.units) ? 2 : 1;
  const int64_t n = nreads / mates;
  std::vector<uint32_t> cnt((size_t)nreads + 1); std::vector<long long> off((size_t)nreads + 1);
  if (nreads) {
    HIPCHK(hipMemcpy(cnt.data(), c->d_ivcnt, (size_t)nreads * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(off.data(), c->d_ivoff, (size_t)nreads * 8, hipMemcpyDeviceToHost));
  }
  int_offsets[0] = 0;
  for (int64_t i = 0; i < n; ++i) {
    int64_t t = 0;
    for (int m = 0; m < mates; ++m) t += cnt[(size_t)(i * mates + m)];
    int_offsets[i + 1] = int_offsets[i] + t;
  }
  if (!ints) return QM_OK;
  if (cap < int_offsets[n]) return fail(QM_E_ARG, "interval buffer too small");
  // the cursor of the chunked allocator may stand up to one chunk behind the buffer's end (a chunk is reserved whole, the
  // overflow check is per read): only what lies inside the allocation is copied -- every recorded interval does
  const int64_t used = c->last.ivTotal < c->d_iv.cap ? c->last.ivTotal : c->d_iv.cap;
  std::vector<qm_sa_interval_hit> all((size_t)used + 1);
  if (used) HIPCHK(hipMemcpy(all.data(), c->d_iv, (size_t)used * sizeof(qm_sa_interval_hit), hipMemcpyDeviceToHost));
  int64_t w = 0;
  for (int64_t r = 0; r < nreads; ++r)
    for (uint32_t j = 0; j < cnt[(size_t)r]; ++j) {
      if (off[(size_t)r] + (long long)j >= used) return fail(QM_E_STATE, "interval list of read %lld lies outside the buffer (internal error)", (long long)r);
      ints[w++] = all[(size_t)(off[(size_t)r] + j)];
    }
  return QM_OK;
}

// ---- the reference's three entry points as calls of their own (include/qmap_rapmap_compat.hpp sits on these) ----------------

static int upload(qm_ctx* c, void* dst, const void* src, size_t bytes) {
  if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  return QM_OK;
}

int qm_collect_reads(qm_ctx* c, const qm_opts* o, int64_t n, const char* seq, const int64_t* off, int64_t* n_intervals) {
  if (!c || n < 0 || (n > 0 && (!seq || !off))) return fail(QM_E_ARG, "bad argument");
  int rc = check_opts(o);
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  static const int64_t zero = 0;
  if (n == 0) off = &zero;
  int32_t maxLen = 0;
  for (int64_t i = 0; i < n; ++i) { const int64_t l = off[i + 1] - off[i]; if (l < 0) return fail(QM_E_ARG, "offsets not monotone"); if (l > maxLen) maxLen = (int32_t)(l > 0x7fffffff ? 0x7fffffff : l); }
  if (maxLen > QM_MAX_LONG_READ_LEN) return fail(QM_E_TOOLONG, "read length %d > %d", maxLen, QM_MAX_LONG_READ_LEN);
  if ((rc = c->d_seq1.ensure(off[n] + 64))) return rc;
  if ((rc = c->d_off1.ensure(n + 1))) return rc;
  if ((rc = upload(c, c->d_off1, off, (size_t)(n + 1) * 8))) return rc;
  if ((rc = upload(c, c->d_seq1, seq, (size_t)off[n]))) return rc;
  RunReq rq; rq.mode = QM_RUN_COLLECT;
  u64 hscal[QM_SC_WORDS];
  begin_call(c);
  if ((rc = run_stage_a(c, o, rq, n, c->d_seq1, c->d_off1, nullptr, nullptr, 8, nullptr, hscal))) return rc;
  if (n_intervals) {
    std::vector<uint32_t> cnt((size_t)n + 1);
    if (n) HIPCHK(hipMemcpy(cnt.data(), c->d_ivcnt, (size_t)n * 4, hipMemcpyDeviceToHost));
    int64_t t = 0; for (int64_t i = 0; i < n; ++i) t += cnt[(size_t)i];
    *n_intervals = t;
  }
  return QM_OK;
}

int qm_fetch_found(qm_ctx* c, uint8_t* found) {
  if (!c || c->last.foundReads < 0) return fail(QM_E_STATE, "no foundHit flags kept by the last call");
  if (!found) return fail(QM_E_ARG, "null buffer");
  HIPCHK(hipSetDevice(c->device));
  if (c->last.foundReads) HIPCHK(hipMemcpy(found, c->d_found, (size_t)c->last.foundReads, hipMemcpyDeviceToHost));
  return QM_OK;
}

int qm_hits_to_mappings(qm_ctx* c, const qm_opts* o, int64_t n, const int32_t* read_len, const int64_t* int_offsets,
                        const qm_sa_interval_hit* ints, int64_t* n_words) {
  if (!c || n < 0 || (n > 0 && (!read_len || !int_offsets))) return fail(QM_E_ARG, "bad argument");
  int rc = check_opts(o);
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  static const int64_t zero = 0;
  if (n == 0) int_offsets = &zero;
  const int64_t ni = int_offsets[n];
  if (ni > 0 && !ints) return fail(QM_E_ARG, "null intervals");
  for (int64_t i = 0; i < n; ++i) {
    if (int_offsets[i + 1] < int_offsets[i]) return fail(QM_E_ARG, "interval offsets not monotone");
    if (read_len[i] < 0 || read_len[i] > QM_MAX_LONG_READ_LEN) return fail(QM_E_TOOLONG, "read length %d > %d", read_len[i], QM_MAX_LONG_READ_LEN);
    int nf = 0, nr = 0; bool seenRc = false;
    for (int64_t j = int_offsets[i]; j < int_offsets[i + 1]; ++j) {
      if (ints[j].query_rc) { ++nr; seenRc = true; } else { ++nf; if (seenRc) return fail(QM_E_ARG, "read %lld: forward-strand intervals must precede the reverse-complement ones", (long long)i); }
      if ((int64_t)(uint32_t)ints[j].end > c->ix->nSA || (uint32_t)ints[j].end < (uint32_t)ints[j].begin) return fail(QM_E_ARG, "read %lld: SA interval out of range", (long long)i);
    }
    if (nf > QM_ICAP + QM_IOVF || nr > QM_ICAP + QM_IOVF) return fail(QM_E_ARG, "read %lld: more than %d intervals on one strand", (long long)i, QM_ICAP + QM_IOVF);
  }
  if ((rc = c->d_ivIn.ensure(ni + 1))) return rc;
  if ((rc = c->d_ivInOff.ensure(n + 1))) return rc;
  if ((rc = c->d_lenIn.ensure(n + 1))) return rc;
  if ((rc = upload(c, c->d_ivIn, ints, (size_t)ni * sizeof(qm_sa_interval_hit)))) return rc;
  if ((rc = upload(c, c->d_ivInOff, int_offsets, (size_t)(n + 1) * 8))) return rc;
  if ((rc = upload(c, c->d_lenIn, read_len, (size_t)n * 4))) return rc;
  RunReq rq; rq.mode = QM_RUN_FROM_INTERVALS; rq.ivIn = c->d_ivIn; rq.ivInOff = c->d_ivInOff; rq.lenIn = c->d_lenIn;
  u64 hscal[QM_SC_WORDS];
  begin_call(c);
  // the kernel walks the reads of one "mate"; seq/off are not touched in this mode (a non-null seq1 keeps the argument checks simple)
  if ((rc = run_stage_a(c, o, rq, n, c->d_lenIn, c->d_ivInOff, nullptr, nullptr, 4, nullptr, hscal))) return rc;
  if (n_words) {
    std::vector<uint32_t> cnt((size_t)n + 1);
    if (n) HIPCHK(hipMemcpy(cnt.data(), c->d_lcnt, (size_t)n * 4, hipMemcpyDeviceToHost));
    int64_t t = 0; for (int64_t i = 0; i < n; ++i) t += cnt[(size_t)i] & 0x7fffffffu;
    *n_words = t;
  }
  return QM_OK;
}

int qm_fetch_read_lists(qm_ctx* c, int64_t* list_offsets, uint64_t* words, int64_t cap) {
  if (!c || c->last.listReads < 0) return fail(QM_E_STATE, "no per-read hit lists kept by the last call");
  if (!list_offsets) return fail(QM_E_ARG, "null list_offsets");
  HIPCHK(hipSetDevice(c->device));
  const int64_t nreads = c->last.listReads;
  std::vector<uint32_t> cnt((size_t)nreads + 1); std::vector<long long> off((size_t)nreads + 1);
  if (nreads) {
    HIPCHK(hipMemcpy(cnt.data(), c->d_lcnt, (size_t)nreads * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(off.data(), c->d_loff, (size_t)nreads * 8, hipMemcpyDeviceToHost));
  }
  list_offsets[0] = 0;
  for (int64_t r = 0; r < nreads; ++r) list_offsets[r + 1] = list_offsets[r] + (int64_t)(cnt[(size_t)r] & 0x7fffffffu);
  if (!words) return QM_OK;
  if (cap < list_offsets[nreads]) return fail(QM_E_ARG, "list buffer too small");
  // the lists sit in bump-allocated chunks: bring the used part of the buffer down once, gather on the host
  const int64_t used = c->last.listWords < c->d_lists.cap ? c->last.listWords : c->d_lists.cap;
  std::vector<uint64_t> all((size_t)used + 1);
  if (used) HIPCHK(hipMemcpy(all.data(), c->d_lists, (size_t)used * 8, hipMemcpyDeviceToHost));
  for (int64_t r = 0; r < nreads; ++r) {
    const int64_t k = (int64_t)(cnt[(size_t)r] & 0x7fffffffu);
    if (k) memcpy(words + list_offsets[r], all.data() + off[(size_t)r], (size_t)k * 8);
  }
  return QM_OK;
}

int qm_merge_lists(qm_ctx* c, const qm_opts* o, int64_t n, const int64_t* loff_left, const uint64_t* words_left, const int64_t* loff_right,
                   const uint64_t* words_right, const uint8_t* found_left, const uint8_t* found_right, const int32_t* len_left,
                   const int32_t* len_right, int64_t* n_hits, qm_counters* counters) {
  if (!c || n < 0 || (n > 0 && (!loff_left || !loff_right || !len_left || !len_right))) return fail(QM_E_ARG, "bad argument");
  int rc = check_opts(o);
  if (rc) return rc;
  if (o->sel_aln && !(found_left && found_right)) return fail(QM_E_ARG, "mergeLeftRightHitsFuzzy needs leftMatches / rightMatches");
  HIPCHK(hipSetDevice(c->device));
  static const int64_t zero = 0;
  if (n == 0) { loff_left = &zero; loff_right = &zero; }
  const int64_t wl = loff_left[n], wr = loff_right[n];
  if ((wl > 0 && !words_left) || (wr > 0 && !words_right)) return fail(QM_E_ARG, "null list words");
  // device image: read 2u = left list of unit u, read 2u + 1 = right list; left words first, right words behind them
  std::vector<uint32_t> cnt((size_t)(2 * n) + 1); std::vector<long long> off((size_t)(2 * n) + 1), o1((size_t)n + 1), o2((size_t)n + 1);
  const bool flags = o->fuzzy || o->sel_aln;
  o1[0] = 0; o2[0] = 0;
  for (int64_t u = 0; u < n; ++u) {
    const int64_t a = loff_left[u + 1] - loff_left[u], b = loff_right[u + 1] - loff_right[u];
    if (a < 0 || b < 0 || a > 0x7ffffffe || b > 0x7ffffffe) return fail(QM_E_ARG, "list offsets not monotone");
    cnt[(size_t)(2 * u)] = (uint32_t)a | ((flags && found_left && found_left[u]) ? 0x80000000u : 0u);
    cnt[(size_t)(2 * u + 1)] = (uint32_t)b | ((flags && found_right && found_right[u]) ? 0x80000000u : 0u);
    off[(size_t)(2 * u)] = loff_left[u]; off[(size_t)(2 * u + 1)] = wl + loff_right[u];
    o1[(size_t)u + 1] = o1[(size_t)u] + len_left[u]; o2[(size_t)u + 1] = o2[(size_t)u] + len_right[u];
  }
  if ((rc = c->d_lcnt.ensure(2 * n + 1))) return rc;
  if ((rc = c->d_loff.ensure(2 * n + 1))) return rc;
  if (c->d_lists.cap < wl + wr + 1) { if ((rc = c->d_lists.ensure(wl + wr + 1))) return rc; }
  if ((rc = c->d_off1.ensure(n + 1))) return rc;
  if ((rc = c->d_off2.ensure(n + 1))) return rc;
  if ((rc = upload(c, c->d_lcnt, cnt.data(), (size_t)(2 * n) * 4))) return rc;
  if ((rc = upload(c, c->d_loff, off.data(), (size_t)(2 * n) * 8))) return rc;
  if ((rc = upload(c, c->d_lists, words_left, (size_t)wl * 8))) return rc;
  if ((rc = upload(c, c->d_lists + wl, words_right, (size_t)wr * 8))) return rc;
  if ((rc = upload(c, c->d_off1, o1.data(), (size_t)(n + 1) * 8))) return rc;
  if ((rc = upload(c, c->d_off2, o2.data(), (size_t)(n + 1) * 8))) return rc;
  HIPCHK(hipMemsetAsync(c->d_scal, 0, QM_SC_WORDS * sizeof(u64), c->stream));
  RunReq rq; rq.mergeOnly = true;
  u64 hscal[QM_SC_WORDS]; long long total = 0;
  begin_call(c);
  if ((rc = run_stage_b(c, o, rq, n, true, nullptr, c->d_off1, nullptr, c->d_off2, hscal, total))) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  c->last.units = n; c->last.hits = total; c->last.paired = true;
  if (n_hits) *n_hits = total;
  if (counters) *counters = counters_from(hscal);
  return QM_OK;
}

int qm_fetch_too_many(qm_ctx* c, uint8_t* too_many) {
  if (!c || c->last.tooManyUnits < 0) return fail(QM_E_STATE, "no tooManyHits flags kept by the last call");
  if (!too_many) return fail(QM_E_ARG, "null buffer");
  HIPCHK(hipSetDevice(c->device));
  if (c->last.tooManyUnits) HIPCHK(hipMemcpy(too_many, c->d_tooMany, (size_t)c->last.tooManyUnits, hipMemcpyDeviceToHost));
  return QM_OK;
}

int qm_map_pairs_stages(qm_ctx* c, const qm_opts* o, int64_t n, const char* seq1, const int64_t* off1, const char* seq2,
                        const int64_t* off2, int64_t* n_hits, qm_counters* counters) {
  if (!seq2 || !off2) return fail(QM_E_ARG, "qm_map_pairs_stages needs both mates");
  RunReq rq; rq.keepIntervals = true; rq.keepFound = true; rq.mergeOnly = true; rq.stageView = true;
  return map_host(c, o, n, seq1, off1, seq2, off2, n_hits, counters, rq);
}

static RunReq stage_req(uint32_t stage_flags) {
  RunReq rq; rq.keepIntervals = !(stage_flags & QM_STAGES_NO_INTERVALS); rq.keepFound = true; rq.mergeOnly = true; rq.stageView = true;
  return rq;
}
int qm_map_pairs_stages_ex(qm_ctx* c, const qm_opts* o, int64_t n, const char* seq1, const int64_t* off1, const char* seq2,
                           const int64_t* off2, uint32_t stage_flags, int64_t* n_hits, qm_counters* counters) {
  if (!seq2 || !off2) return fail(QM_E_ARG, "qm_map_pairs_stages_ex needs both mates");
  return map_host(c, o, n, seq1, off1, seq2, off2, n_hits, counters, stage_req(stage_flags));
}
int qm_map_pairs_stages_packed(qm_ctx* c, const qm_opts* o, int64_t n, const uint8_t* pk1, const int64_t* off1, const qm_pack_exc* exc1, int64_t nexc1,
                               const uint8_t* pk2, const int64_t* off2, const qm_pack_exc* exc2, int64_t nexc2, uint32_t stage_flags, int64_t* n_hits, qm_counters* counters) {
  if (!pk2 || !off2) return fail(QM_E_ARG, "qm_map_pairs_stages_packed needs both mates");
  return map_packed(c, o, n, pk1, off1, exc1, nexc1, pk2, off2, exc2, nexc2, n_hits, counters, stage_req(stage_flags));
}

// layout of a qm_fetch_stages arena: eight arrays, each aligned to 64 bytes
namespace {
struct StageLayout { size_t ivOff, iv, found, listOff, words, hitOff, hits, tooMany, total; };
StageLayout stage_layout(int64_t nreads, int64_t n, int64_t nIv, int64_t nWords, int64_t nHits) {
  StageLayout L; size_t p = 0;
  auto take = [&](size_t bytes) { const size_t at = p; p += (bytes + 63) & ~(size_t)63; return at; };
  L.ivOff = take((size_t)(nreads + 1) * 8); L.iv = take((size_t)(nIv + 1) * sizeof(qm_sa_interval_hit)); L.found = take((size_t)nreads + 1);
  L.listOff = take((size_t)(nreads + 1) * 8); L.words = take((size_t)(nWords + 1) * 8);
  L.hitOff = take((size_t)(n + 1) * 8); L.hits = take((size_t)(nHits + 1) * sizeof(qm_hit)); L.tooMany = take((size_t)n + 1);
  L.total = p;
  return L;
}
}  // namespace

int qm_stage_bytes(qm_ctx* c, int64_t* bytes) {
  if (!c || !bytes) return fail(QM_E_ARG, "null argument");
  if (c->last.stUnits < 0 || c->last.stReads < 0 || c->last.units != c->last.stUnits) return fail(QM_E_STATE, "qm_stage_bytes: the last call on this context was not qm_map_pairs_stages");
  *bytes = (int64_t)stage_layout(c->last.stReads, c->last.stUnits, c->h_tot[0], c->h_tot[1], c->last.hits).total;
  return QM_OK;
}

int qm_fetch_stages(qm_ctx* c, void* arena, int64_t arena_bytes, qm_stage_view* v) {
  if (!c || !arena || !v) return fail(QM_E_ARG, "null argument");
  if (c->last.stUnits < 0 || c->last.stReads < 0 || c->last.units != c->last.stUnits) return fail(QM_E_STATE, "qm_fetch_stages: the last call on this context was not qm_map_pairs_stages");
  HIPCHK(hipSetDevice(c->device));
  const int64_t nreads = c->last.stReads, n = c->last.stUnits, nIv = c->h_tot[0], nWords = c->h_tot[1], nHits = c->last.hits;
  const StageLayout L = stage_layout(nreads, n, nIv, nWords, nHits);
  if ((int64_t)L.total > arena_bytes) return fail(QM_E_ARG, "qm_fetch_stages: arena of %lld bytes, %lld needed (qm_stage_bytes)", (long long)arena_bytes, (long long)L.total);
  int rc;
  if ((rc = c->d_ivC.ensure(nIv + 1, nIv / 4))) return rc;
  if ((rc = c->d_wordsC.ensure(nWords + 1, nWords / 4))) return rc;
  HIPCHK(qmk_stage_gather(nreads, c->d_ivcnt, c->d_ivoff, c->d_iv, c->d_ivcsr, c->d_ivC, c->d_lcnt, c->d_loff, (const unsigned long long*)c->d_lists, c->d_lcsr,
                          (unsigned long long*)c->d_wordsC, c->stream));
  unsigned char* A = (unsigned char*)arena;
  auto down = [&](size_t at, const void* src, size_t bytes) -> hipError_t {
    return bytes ? hipMemcpyAsync(A + at, src, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
  };
  HIPCHK(down(L.ivOff, c->d_ivcsr, (size_t)(nreads + 1) * 8));
  HIPCHK(down(L.iv, c->d_ivC, (size_t)nIv * sizeof(qm_sa_interval_hit)));
  HIPCHK(down(L.found, c->d_found, (size_t)nreads));
  HIPCHK(down(L.listOff, c->d_lcsr, (size_t)(nreads + 1) * 8));
  HIPCHK(down(L.words, c->d_wordsC, (size_t)nWords * 8));
  HIPCHK(down(L.hitOff, c->d_offs, (size_t)(n + 1) * 8));
  HIPCHK(down(L.hits, c->d_hits, (size_t)nHits * sizeof(qm_hit)));
  HIPCHK(down(L.tooMany, c->d_tooMany, (size_t)n));
  HIPCHK(hipStreamSynchronize(c->stream));
  v->n_units = n; v->n_reads = nreads;
  v->iv_off = (const int64_t*)(A + L.ivOff); v->iv = (const qm_sa_interval_hit*)(A + L.iv); v->found = A + L.found;
  v->list_off = (const int64_t*)(A + L.listOff); v->words = (const uint64_t*)(A + L.words);
  v->hit_off = (const int64_t*)(A + L.hitOff); v->hits = (const qm_hit*)(A + L.hits); v->too_many = A + L.tooMany;
  if (nreads == 0) { ((int64_t*)(A + L.ivOff))[0] = 0; ((int64_t*)(A + L.listOff))[0] = 0; }
  if (n == 0) ((int64_t*)(A + L.hitOff))[0] = 0;
  return QM_OK;
}

void* qm_pinned_alloc(int64_t bytes) {
  void* p = nullptr;
  return hipHostMalloc(&p, bytes > 0 ? (size_t)bytes : 64, hipHostMallocPortable) == hipSuccess ? p : nullptr;
}
void qm_pinned_free(void* p) { if (p) hipHostFree(p); }

int qm_ctx_stat(const qm_ctx* c, int which, int64_t* value) {
  if (!c || !value) return fail(QM_E_ARG, "null argument");
  const CallStats& s = c->stats;
  switch (which) {
    case QM_STAT_RELAUNCHES: *value = s.relaunches; break;
    case QM_STAT_LIST_WORDS: *value = c->d_lists.cap; break;
    case QM_STAT_SLOW_READS: *value = s.slowReads; break;
    case QM_STAT_LEAN_READS: *value = s.leanReads; break;
    case QM_STAT_LEAN_DEFERRED: *value = s.leanDeferred; break;
    case QM_STAT_SKIPPED_READS: *value = s.skipped; break;
    case QM_STAT_SEL_QUESTIONS: *value = s.selQuestions; break;
    case QM_STAT_KSW2_ALIGNMENTS: *value = s.kswTasks; break;
    case QM_STAT_STRIP_ALIGNMENTS: *value = s.stripTasks; break;
    case QM_STAT_PAIR_KERNEL_PAIRS: *value = s.duoPairs; break;
    case QM_STAT_PAIRS_MERGED: *value = s.duoMerged; break;
    case QM_STAT_N_PASS_READS: *value = s.nPass; break;
    case QM_STAT_DEFER_DIRTY: case QM_STAT_DEFER_HOMOPOLYMER: case QM_STAT_DEFER_WIDE: case QM_STAT_DEFER_BOTH_STRANDS: *value = s.defer[which - QM_STAT_DEFER_DIRTY]; break;
    default: return fail(QM_E_ARG, "unknown statistic %d", which);
  }
  return QM_OK;
}

int qm_fetch_skipped(const qm_ctx* c, int64_t* reads, int32_t* codes, int64_t cap, int64_t* total) {
  if (!c || !total) return fail(QM_E_ARG, "null argument");
  *total = c->stats.skipped;
  const int64_t n = (int64_t)c->stats.skipList.size() < cap ? (int64_t)c->stats.skipList.size() : cap;
  for (int64_t i = 0; i < n; ++i) {
    if (reads) reads[i] = (int64_t)(c->stats.skipList[(size_t)i] & ((1ULL << 56) - 1));
    if (codes) codes[i] = (int32_t)(c->stats.skipList[(size_t)i] >> 56);
  }
  return QM_OK;
}

int qm_last_kernel_ms(const qm_ctx* c, double* map_ms, double* total_ms) {
  if (!c || c->last.units < 0) return fail(QM_E_STATE, "no mapping result");
  if (map_ms) *map_ms = c->last.mapMs;
  if (total_ms) *total_ms = c->last.totalMs;
  return QM_OK;
}

}  // extern "C"

// the equivalence-class table (qm_eqc_*): its host driver reads the context's last result
#include "qm_eqc_host.inl"
#include "qm_quant_host.inl"
#include "qm_boot_host.inl"
#include "qm_fld_host.inl"
#include "qm_lib_host.inl"
#include "qm_gcb_host.inl"
#include "qm_sqb_host.inl"
#include "qm_psb_host.inl"
