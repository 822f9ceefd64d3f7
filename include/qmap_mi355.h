/* qmap_mi355.h -- C ABI of libqmap_mi355.so, the MI355X-native drop-in for the
 * `rapmap quasimap` hot path (RapMap v0.6.0).
 *
 * RapMap has no FFI/plugin registry: its callers compile three C++ template
 * entry points into themselves.  This header is the
 * batched, language-neutral face of the same three steps; each entry point
 * cites the reference interface it replaces (paths relative to the reference
 * tree).  Plain pointers and sizes only; no C++/torch types.  All functions
 * return 0 on success or a negative qm_status; none of them calls exit().
 *
 * One call of qm_map_pairs() == for every read pair i:
 *     SACollector::operator()(left)  ; SACollector::operator()(right)       include/SACollector.hpp:108-362
 *     hit_manager::hitsToMappingsSimple(..., PAIRED_END_LEFT / _RIGHT, ...)  src/HitManager.cpp:691-882
 *     utils::mergeLeftRightHits(...)                                         include/RapMapUtils.hpp:1185-1264
 *     + the per-pair bookkeeping of processReadsPairSA                       src/RapMapSAMapper.cpp:461-551,684-701
 * executed on the GPU: one 64-lane wavefront per read for the first two steps, one thread per pair for the merge.
 */
#ifndef QMAP_MI355_H
#define QMAP_MI355_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum qm_status {
  QM_OK = 0,
  QM_E_ARG = -1,         /* bad argument */
  QM_E_IO = -2,          /* index file missing / malformed */
  QM_E_NOGPU = -3,       /* no HIP device, or HIP call failed */
  QM_E_UNSUPPORTED = -4, /* option / index variant not implemented on the device path */
  QM_E_TOOLONG = -5,     /* a read is longer than QM_MAX_LONG_READ_LEN */
  QM_E_NOMEM = -6,
  QM_E_STATE = -7,       /* call order (e.g. fetch before map) */
  QM_E_FORMAT = -8       /* malformed FASTA/FASTQ input */
} qm_status;

/* Reads of up to QM_MAX_READ_LEN characters are mapped by the main kernels (64-character slot classes 2 / 3 / 4 / 8).  Longer
 * reads of a batch -- up to QM_MAX_LONG_READ_LEN -- are set aside by the main launch and mapped by a second, small launch of
 * 32-slot kernels (the reference takes any std::string, include/SACollector.hpp:108); with -s the same happens in the
 * collector pass and the alignment kernel runs in its long-image editions (with --dpBandwidth beyond 97 or negative: on blocks
 * in device memory, a ring that holds every column of a 2048-base alignment -- slow, and rare).  A read beyond QM_MAX_LONG_READ_LEN is
 * skipped, not mapped (round 5): it comes back without hits and on the skip list (qm_fetch_skipped), the batch goes on; the stage
 * entries that take caller-supplied lengths (qm_hits_to_mappings, ...) still answer QM_E_TOOLONG. */
#define QM_MAX_READ_LEN 512
#define QM_MAX_LONG_READ_LEN 2048

/* Mirrors MappingOpts (src/RapMapSAMapper.cpp:114-152) for the fields that
 * reach the hot path.  Defaults (qm_opts_default) == `rapmap quasimap` defaults
 * (src/RapMapSAMapper.cpp:992-1023,1113-1114). */
typedef struct qm_opts {
  int32_t sensitive;     /* 1 unless --noSensitive (disableNIP, SACollector.hpp:40)        */
  int32_t strict_check;  /* 1 unless --noStrictCheck (SACollector.hpp:61)                  */
  int32_t max_num_hits;  /* -m, 200                                                       */
  int32_t no_orphans;    /* --noOrphans                                                   */
  int32_t no_dovetail;   /* --noDovetail                                                  */
  int32_t fuzzy;         /* -f  mergeLeftRightHitsFuzzy, include/RapMapUtils.hpp:864-1183   */
  int32_t max_interval;  /* SACollector::setMaxInterval, 1000 (SACollector.hpp:54,77)     */
  int32_t sel_aln;       /* -s  selective alignment (src/RapMapSAMapper.cpp:554-667)        */
  double quasi_cov;      /* -z  (SACollector::setCoverageRequirement)                     */
  /* sub-options of -s (src/RapMapSAMapper.cpp:1011-1023,1135-1175); read only when sel_aln != 0 */
  int32_t hard_filter;        /* --hardFilter                                             */
  int32_t match_score;        /* --ma, 2                                                  */
  int32_t mismatch_penalty;   /* --mm, -4                                                 */
  int32_t gap_open;           /* --go, 4                                                  */
  int32_t gap_extend;         /* --ge, 2                                                  */
  int32_t dp_bandwidth;       /* --dpBandwidth, 15                                        */
  int32_t max_mmp_extension;  /* --maxMMPExtension, 7                                     */
  int32_t aln_policy;         /* 0 default, 1 --mimicBT2, 2 --mimicStrictBT2              */
  double min_score_fraction;  /* --minScoreFrac, 0.65                                     */
  double consensus_slack;     /* --consensusSlack, 0.2; a negative value -f gives MappingConfig::consensusFraction = f directly */
} qm_opts;

/* POD image of rapmap::utils::QuasiAlignment (include/RapMapUtils.hpp:399-502),
 * restricted to the fields that are defined on this path.  For orphan / single-end
 * hits the reference leaves matePos and mateLen uninitialised; here they are 0. */
typedef struct qm_hit {
  uint32_t tid;
  int32_t pos;
  int32_t mate_pos;
  uint32_t frag_len;
  uint32_t read_len;
  uint32_t mate_len;
  uint8_t fwd;
  uint8_t mate_is_fwd;
  uint8_t is_paired;
  uint8_t mate_status; /* MateStatus: 0 SINGLE_END 1 PE_LEFT 2 PE_RIGHT 3 PE_PAIRED (RapMapUtils.hpp:356-362) */
  int32_t aln_score;   /* alnScore_, 0 without -s */
} qm_hit;

/* rapmap::utils::HitCounters (include/RapMapUtils.hpp:208-216) + mapped units */
typedef struct qm_counters {
  uint64_t pe_hits, se_hits, tot_hits, num_reads, too_many_hits, mapped;
} qm_counters;

/* rapmap::utils::SAIntervalHit<OffsetT> (include/RapMapUtils.hpp:516-525) + which list it sits in.  begin / end are the device's
 * 32-bit offsets: for a BigSA index (OffsetT = int64_t in the reference) read them as uint32_t */
typedef struct qm_sa_interval_hit {
  int32_t begin, end;
  uint32_t len, query_pos;
  uint8_t query_rc;
  uint8_t list; /* 0 left-fwd, 1 left-rc, 2 right-fwd, 3 right-rc */
  uint16_t pad;
} qm_sa_interval_hit;

typedef struct qm_index_info {
  int32_t k;
  int32_t big_sa;
  int32_t perfect_hash;
  int32_t pad;
  int64_t text_len;
  int64_t n_txps;
  int64_t n_keys;
} qm_index_info;

typedef struct qm_index qm_index; /* host image of the on-disk quasi-index */
typedef struct qm_ctx qm_ctx;     /* one device context: index replica in HBM + work buffers */

const char* qm_last_error(void);
const char* qm_version(void);
int qm_opts_default(qm_opts* o);

/* RapMapSAIndex<int32_t, RegHashT>::load (src/RapMapSAIndex.cpp:97-176): reads
 * header.json, sa.bin, txpInfo.bin, rsd.bin and hash.bin -- or, for a perfect-hash (-p) index
 * (RapMapSAIndex<int32_t, PerfectHashT>, include/FrugalBooMap.hpp), hash_info.bph + hash_info.val --
 * of a "q5" index directory (files are mmap'd, not deserialised). */
int qm_index_open(const char* dir, qm_index** out);
int qm_index_close(qm_index* ix);
int qm_index_info_get(const qm_index* ix, qm_index_info* info);
const char* qm_index_txp_name(const qm_index* ix, int64_t tid); /* rmi.txpNames[tid] */
int64_t qm_index_txp_len(const qm_index* ix, int64_t tid);      /* rmi.txpLens[tid]  */
/* Read-only views of rmi.seq (the '$'-separated text) and rmi.txpOffsets (include/RapMapSAIndex.hpp:70-82);
 * valid until qm_index_close.  The offsets are UNSIGNED 32-bit values (read them as uint32_t for a BigSA index, whose text may
 * pass 2^31 characters; the int64 vectors of such an index are narrowed at open and its text must stay below 2^32 - 2). */
int qm_index_arrays(const qm_index* ix, const uint8_t** text, int64_t* text_len, const int32_t** txp_offsets,
                    int64_t* n_txps);
/* The other arrays of an open index as the library holds them, for inspection and cross-checks (profiles/r04/big_index_crosscheck.py
 * holds them against the oracle's independent numpy reader and the reference's own container): which = QM_RAW_SA -- the suffix
 * array as uint32_t[count] (a BigSA index's int64 entries narrowed at open), QM_RAW_HASH -- the dense hash's records, count x 16
 * bytes {uint64 k-mer word, uint32 lb, uint32 ub} in file order (NULL / 0 for a -p index), QM_RAW_COMPLETE_LENS -- uint32_t[count]. */
enum { QM_RAW_SA = 0, QM_RAW_HASH = 1, QM_RAW_COMPLETE_LENS = 2 };
int qm_index_raw(const qm_index* ix, int which, const void** data, int64_t* count);

/* Replicates the index into the HBM of `device_id` as flat SoA arrays and
 * allocates the per-context work buffers.  One ctx per GPU / per host thread (a context is not thread-safe); the
 * contexts of one index on one device share a single replica, which is freed with the last of them.  Destroy the
 * contexts before closing the index. */
int qm_ctx_create(const qm_index* ix, int device_id, qm_ctx** out);
/* flags: QM_CTX_PH_COMPACT -- a perfect-hash (-p) index keeps the reference's frugal structure on the device (re-blocked
 * BooPHF levels walked per lookup, include/BooPHF.hpp:971-1009, + one 16-byte record per k-mer: 1.3 GB for 80 M k-mers).
 * By default a -p index is expanded at load time into the same one-sector bucket table a dense index gets (8.6 GB), after
 * every record has been looked up through the BooPHF walk itself: identical answers, a single HBM round trip per lookup. */
/* QM_CTX_NO_PAIR_KERNEL (round 6) -- paired reads of up to 128 characters take qm_lean_kernel alone instead of the pair kernel / a part
 * of each kind (tests, A/B timing; the answers are the same).  QM_CTX_WIDE_READS -- build the wide extension table (reads of 129 .. 256
 * characters: 64 bytes per suffix-array entry) with the replica instead of inside the first call that has such reads. */
enum { QM_CTX_PH_COMPACT = 1, QM_CTX_NO_PAIR_KERNEL = 2, QM_CTX_WIDE_READS = 4 };
int qm_ctx_create_ex(const qm_index* ix, int device_id, uint32_t flags, qm_ctx** out);
int qm_ctx_destroy(qm_ctx* ctx);
int64_t qm_ctx_device_bytes(const qm_ctx* ctx);

/* Map n read pairs held in HOST memory.  seqX = concatenated read bytes (ASCII,
 * any case, N allowed), offX[n+1] = byte offsets.  Results stay in the context;
 * *n_hits receives the total number of hits.  counters may be NULL.
 * The buffers may be pageable: the characters are uploaded in chunks on a copy
 * stream and every chunk is mapped as soon as it has arrived, so transfer and
 * mapping overlap inside one call; nothing is in flight once the call returns. */
int qm_map_pairs(qm_ctx* ctx, const qm_opts* opts, int64_t n, const char* seq1, const int64_t* off1,
                 const char* seq2, const int64_t* off2, int64_t* n_hits, qm_counters* counters);
/* Same for single-end reads (processReadsSingleSA, src/RapMapSAMapper.cpp:232-250). */
int qm_map_reads(qm_ctx* ctx, const qm_opts* opts, int64_t n, const char* seq, const int64_t* off,
                 int64_t* n_hits, qm_counters* counters);
/* Same, with the inputs already resident in this device's memory (d_* are device
 * pointers; seq2/off2 NULL for single-end).  `max_read_len` bounds every read. */
int qm_map_device(qm_ctx* ctx, const qm_opts* opts, int64_t n, const void* d_seq1, const void* d_off1,
                  const void* d_seq2, const void* d_off2, int32_t max_read_len, int64_t* n_hits,
                  qm_counters* counters);
/* ---- 2-bit packed reads (replaces the per-record std::strings of src/FastxParser.cpp:229-328 on the way
 * to the device).  A host-buffer call moves 100 bytes per 100-bp read over PCIe; packed it moves 26.  The format keeps EVERY
 * character (the collector treats lower case, N, IUPAC codes and U differently, include/SACollector.hpp:176-192,498-536):
 *   read i's characters [off[i], off[i+1]) sit four to a byte -- character j of a group in bits 2j, 2j+1; A 0, C 1, G 2, T 3,
 *   upper case only -- from byte qm_packed_offset(off, i) = (off[i] >> 2) + i on (reads never share a byte: any number of
 *   threads may pack different reads of one batch side by side);
 *   every other character is an EXCEPTION {position in the concatenated sequence, character} and has code 0 in the packed bytes.
 * The device unpacks into the ASCII image the kernels read (one thread per group of four, then one per exception) and maps as
 * qm_map_pairs / qm_map_reads do: same results, bit for bit.  qm_pack_reads is the host-side packer (the ingest engine packs
 * in its copy tasks with the same routine); QM_E_ARG when the exceptions outgrow exc_cap (callers then send the plain characters). */
typedef struct qm_pack_exc { uint32_t pos; uint32_t ch; } qm_pack_exc;
int64_t qm_packed_offset(const int64_t* off, int64_t i);   /* (off[i] >> 2) + i: where read i's packed bytes start */
int64_t qm_packed_bytes(const int64_t* off, int64_t n);    /* (off[n] >> 2) + n + 8: bytes a packed batch of n reads takes */
int qm_pack_reads(const char* seq, const int64_t* off, int64_t n, uint8_t* packed, qm_pack_exc* exc, int64_t exc_cap, int64_t* n_exc);
int qm_map_pairs_packed(qm_ctx* ctx, const qm_opts* opts, int64_t n, const uint8_t* packed1, const int64_t* off1, const qm_pack_exc* exc1,
                        int64_t n_exc1, const uint8_t* packed2, const int64_t* off2, const qm_pack_exc* exc2, int64_t n_exc2,
                        int64_t* n_hits, qm_counters* counters);
int qm_map_reads_packed(qm_ctx* ctx, const qm_opts* opts, int64_t n, const uint8_t* packed, const int64_t* off, const qm_pack_exc* exc,
                        int64_t n_exc, int64_t* n_hits, qm_counters* counters);
/* Copy the results of the last map call to host memory:
 * hit_offsets[n+1] (exclusive prefix sum), hits[n_hits].  Large results come
 * down through pinned staging buffers and are placed by several host threads. */
int qm_fetch_hits(qm_ctx* ctx, int64_t* hit_offsets, qm_hit* hits);
/* The same into PAGE-LOCKED destination memory (hipHostMalloc / hipHostRegister): straight DMA, no staging, no host copy. */
int qm_fetch_hits_pinned(qm_ctx* ctx, int64_t* hit_offsets, qm_hit* hits);
/* Device pointers of the same arrays (valid until the next map call on ctx). */
int qm_result_device(qm_ctx* ctx, const void** d_hit_offsets, const void** d_hits);

/* ---- the reference's three entry points as calls of their own ---------------------------------------------------------
 * RapMap's callers (and Salmon) drive the path per read through three C++ entry points; include/qmap_rapmap_compat.hpp
 * gives them back with the reference's signatures and fills them from the batched calls below.  Each call works on a
 * whole batch; results stay in the context until the next call on it.
 *
 * (1) SACollector::operator()(read, saSearcher, hcInfo)        include/SACollector.hpp:108-362
 *     qm_collect_reads: n reads in, per read the SA-interval hits (HitCollectorInfo::fwdSAInts then rcSAInts,
 *     include/HitManager.hpp:59-72) and the call's return value (foundHit).  opts: sensitive, strict_check, quasi_cov,
 *     max_interval, and with sel_aln the chain-scoring collector (enableChainScoring / setMaxMMPExtension).
 *     qm_fetch_intervals: int_offsets[n+1], ints[int_offsets[n]] (ints = NULL: offsets only); the `list` field tells the
 *     strand (and, after qm_map_pairs / qm_map_pairs_stages on a context with qm_ctx_set_debug, the mate: a pair's four lists
 *     follow each other).  No cap on the number of intervals.
 * (2) hit_manager::hitsToMappingsSimple(rmi, mc, mateStatus, hcinfo, hits)   include/HitManager.hpp:130-135, src/HitManager.cpp:691-882
 *     qm_hits_to_mappings: per read its length and its SA-interval hits (forward-strand records first) in, the read's hit
 *     list out.  opts: fuzzy keeps both orientations of a transcript (what the -f merge consumes); sel_aln = MappingConfig
 *     {doChaining, considerMultiPos} with consensus_slack.  qm_fetch_read_lists: list_offsets[n+1], words[].
 *     List words without sel_aln: one per hit, ascending, tid << 33 | isRC << 32 | (uint32) hitPos.
 *     With sel_aln: per hit  tid | primaryRC << 32 | chainStatus << 33 | nP << 36,  then  (uint32) pos | nO << 32,
 *     then nP positions of the surviving orientation (QuasiAlignment::allPositions) and nO of the other
 *     (oppositeStrandPositions), each in the low 32 bits of a word.
 * (3) utils::mergeLeftRightHits / mergeLeftRightHitsFuzzy          include/RapMapUtils.hpp:1185-1264, :864-1183
 *     qm_merge_lists: per pair the two mates' lists (same word format), their lengths and -- for the fuzzy merge
 *     (opts.fuzzy or opts.sel_aln) -- leftMatches / rightMatches; jointHits come back through qm_fetch_hits, the
 *     tooManyHits out-parameter through qm_fetch_too_many (bit 0; bit 1: the mates shared a transcript), the HitCounters the merge bumps (peHits, seHits, tooManyHits)
 *     in `counters`.  Nothing of the caller's bookkeeping that follows the merge in processReadsPairSA is applied
 *     (src/RapMapSAMapper.cpp:534-551,684-701).  With sel_aln the hits' aln_score carries the chain statuses
 *     (left | right << 4; rapmap::utils::ChainStatus), not a score: the merge does not align.
 * qm_map_pairs_stages = (1)-(3) for a batch of pairs in one fused pass, every stage's output kept: intervals
 * (qm_fetch_intervals, four lists per pair), foundHit (qm_fetch_found, [2n]: left, right, left, ...), per-read lists
 * (qm_fetch_read_lists, [2n+1] offsets), merge results (qm_fetch_hits, qm_fetch_too_many). */
int qm_ctx_set_debug(qm_ctx* ctx, int keep_intervals);   /* fused calls keep the SA-interval hits for qm_fetch_intervals */
int qm_collect_reads(qm_ctx* ctx, const qm_opts* opts, int64_t n, const char* seq, const int64_t* off, int64_t* n_intervals);
int qm_fetch_intervals(qm_ctx* ctx, int64_t* int_offsets, qm_sa_interval_hit* ints, int64_t cap);
int qm_fetch_found(qm_ctx* ctx, uint8_t* found);
int qm_hits_to_mappings(qm_ctx* ctx, const qm_opts* opts, int64_t n, const int32_t* read_len, const int64_t* int_offsets,
                        const qm_sa_interval_hit* ints, int64_t* n_words);
int qm_fetch_read_lists(qm_ctx* ctx, int64_t* list_offsets, uint64_t* words, int64_t cap);
int qm_merge_lists(qm_ctx* ctx, const qm_opts* opts, int64_t n, const int64_t* loff_left, const uint64_t* words_left,
                   const int64_t* loff_right, const uint64_t* words_right, const uint8_t* found_left, const uint8_t* found_right,
                   const int32_t* len_left, const int32_t* len_right, int64_t* n_hits, qm_counters* counters);
int qm_fetch_too_many(qm_ctx* ctx, uint8_t* too_many);
int qm_map_pairs_stages(qm_ctx* ctx, const qm_opts* opts, int64_t n, const char* seq1, const int64_t* off1, const char* seq2,
                        const int64_t* off2, int64_t* n_hits, qm_counters* counters);
/* Round 6: the same pass for callers that do not look inside the collector's SA-interval records -- the reference's own caller hands its
 * HitCollectorInfo straight on to hitsToMappingsSimple (src/RapMapSAMapper.cpp:466-486) -- and / or keep their batches 2-bit packed:
 * QM_STAGES_NO_INTERVALS leaves the interval arrays of the stage view empty (every read's count 0; foundHit, lists, hits and tooMany as
 * before), which lets the pass run on the pair / lean stage-A kernels and brings half the bytes down; _packed takes the reads as
 * qm_map_pairs_packed does (26 bytes up per 100-bp read instead of 100).  stage_flags 0 = qm_map_pairs_stages. */
enum { QM_STAGES_NO_INTERVALS = 1 };
int qm_map_pairs_stages_ex(qm_ctx* ctx, const qm_opts* opts, int64_t n, const char* seq1, const int64_t* off1, const char* seq2,
                           const int64_t* off2, uint32_t stage_flags, int64_t* n_hits, qm_counters* counters);
int qm_map_pairs_stages_packed(qm_ctx* ctx, const qm_opts* opts, int64_t n, const uint8_t* packed1, const int64_t* off1, const qm_pack_exc* exc1,
                               int64_t n_exc1, const uint8_t* packed2, const int64_t* off2, const qm_pack_exc* exc2, int64_t n_exc2,
                               uint32_t stage_flags, int64_t* n_hits, qm_counters* counters);
/* Everything qm_map_pairs_stages kept, brought to the host in ONE go (round 4; what a caller of the reference's per-read call
 * surface needs for a parser chunk of ~10 000 pairs -- src/RapMapSAMapper.cpp:853 -- where five separate fetches, each a
 * synchronous copy of a bump-allocated device buffer, cost far more than the mapping itself).  The per-read interval records
 * and list words are compacted into CSR order ON THE DEVICE (scan + gather), then the eight arrays come down with asynchronous
 * copies on the context's stream and one synchronisation, laid out in an arena the CALLER owns -- page-locked memory
 * (qm_pinned_alloc) makes the copies true DMA; pageable memory works, slower.  qm_stage_bytes says how large the arena must be
 * for the last qm_map_pairs_stages call.  The view's pointers point into the arena.
 *   iv_off[n_reads + 1] / iv[]       per READ (2u = left mate of pair u, 2u + 1 = right): SA-interval hits, forward strand first
 *   found[n_reads]                   SACollector::operator()'s return value
 *   list_off[n_reads + 1] / words[]  per read: hitsToMappingsSimple's list ("List words" above)
 *   hit_off[n_units + 1] / hits[]    per pair: the merge's jointHits;  too_many[n_units]: bit 0 tooManyHits, bit 1 shared transcript */
typedef struct qm_stage_view {
  int64_t n_units, n_reads;
  const int64_t* iv_off; const qm_sa_interval_hit* iv; const uint8_t* found;
  const int64_t* list_off; const uint64_t* words;
  const int64_t* hit_off; const qm_hit* hits; const uint8_t* too_many;
} qm_stage_view;
int qm_stage_bytes(qm_ctx* ctx, int64_t* bytes);
int qm_fetch_stages(qm_ctx* ctx, void* arena, int64_t arena_bytes, qm_stage_view* view);
/* Page-locked host memory for callers that have no HIP runtime of their own to ask (input buffers of the qm_map_* calls,
 * arenas of qm_fetch_stages): hipHostMalloc / hipHostFree. */
void* qm_pinned_alloc(int64_t bytes);
void qm_pinned_free(void* p);

/* Timing of the dominant kernel of the last map call, measured with HIP events on
 * the context's stream (milliseconds); n_launches kernels were timed. */
int qm_last_kernel_ms(const qm_ctx* ctx, double* map_kernel_ms, double* total_ms);

/* Diagnostics of the last map call on ctx (tests, tuning): which = QM_STAT_RELAUNCHES -- how often stage A was run again
 * because the per-read hit lists outgrew their buffer (the buffer is grown and the batch redone; results are unaffected),
 * QM_STAT_LIST_WORDS -- capacity of that buffer in 8-byte words, QM_STAT_SLOW_READS -- reads that took the per-read
 * overflow path of -s (more suffixes than the wave's scratch holds). */
enum { QM_STAT_RELAUNCHES = 0, QM_STAT_LIST_WORDS = 1, QM_STAT_SLOW_READS = 2, QM_STAT_LEAN_READS = 3, QM_STAT_LEAN_DEFERRED = 4, QM_STAT_SKIPPED_READS = 5,
       QM_STAT_SEL_QUESTIONS = 6,    /* -s: alignments the reference would look at beyond PERFECT chains (one per hit and mate) ... */
       QM_STAT_KSW2_ALIGNMENTS = 7,  /* ... the ksw2 alignments the device ran for them (the others: alignment-cache hits, ungapped chains, answers known without ksw2) */
       QM_STAT_STRIP_ALIGNMENTS = 8, /* ... and the alignments answered by the exact strip DP instead (gapless path within q + 7 e of the best possible) */
       QM_STAT_PAIR_KERNEL_PAIRS = 9, /* pairs the pair kernel (both mates in one wavefront, merged there) was launched over; -1: not used.  An unsplit call only
                                         (a call mapped in parts reports QM_STAT_LEAN_READS / _DEFERRED summed over its parts and -1 here) */
       QM_STAT_PAIRS_MERGED = 10,    /* ... of which it merged itself (the others had a mate left to the general kernel, or the call kept lists) */
       /* why the reads of QM_STAT_LEAN_DEFERRED were left to the general kernel (they add up to it): */
       QM_STAT_DEFER_DIRTY = 11,     /* a character that is not A C G T (an N ...), or more characters than the kernel's lanes hold */
       QM_STAT_DEFER_HOMOPOLYMER = 12, /* a window of k equal bases (isHomoPolymer, include/Kmer.hpp:484-487) */
       QM_STAT_DEFER_WIDE = 13,      /* an SA interval wider than the kernel's lanes, more suffixes / intervals than its stash, a match beyond its extension table */
       QM_STAT_DEFER_BOTH_STRANDS = 14, /* k-mers of the other orientation seen on the way: the reference maps the other strand as well (SACollector.hpp:258,271) */
       QM_STAT_N_PASS_READS = 15 };  /* reads with N's that the N-aware second pass of stage A mapped (it runs when QM_NPASS_MIN reads or more -- 2 048 -- were left
                                        for a character outside A C G T; such k-mers are stepped over, SACollector.hpp:172-181,497-512).  They are not part of
                                        QM_STAT_LEAN_DEFERRED or QM_STAT_DEFER_DIRTY, which count what the general kernel took */
int qm_ctx_stat(const qm_ctx* ctx, int which, int64_t* value);

/* Reads of the last map call on ctx that were SKIPPED, not mapped (round 5; before, one such read failed the whole batch): a read
 * longer than QM_MAX_LONG_READ_LEN characters (code 1: the reference takes any std::string, include/SACollector.hpp:108 -- the
 * device kernels' longest slot class does not), a read whose SA-interval lists outgrow the per-wave scratch (code 2: only with
 * max_interval above its default of 1000, include/SACollector.hpp:54,77).  Such a read has an empty result -- no intervals, no
 * hits, foundHit false; its mate is mapped as usual -- and everything else in the batch is mapped as if it were not there.
 * *total = how many there were; the first min(total, cap, 4096) are listed: reads[i] = index of the read in the call (paired
 * calls: 2 * pair + mate), codes[i] as above.  Either array may be null. */
int qm_fetch_skipped(const qm_ctx* ctx, int64_t* reads, int32_t* codes, int64_t cap, int64_t* total);

/* `rapmap quasiindex [-p]` (src/RapMapSAIndexer.cpp:449-819): FASTA -> q5 index directory readable by
 * qm_index_open and by the reference (sa.bin, txpInfo.bin, rsd.bin and -- with perfect_hash --
 * hash_info.bph / hash_info.val come out byte-identical to the reference's).  A text of more than
 * 2^31 - 2 characters gets the reference's int64 form ("BigSA": true: 8-byte transcript starts, suffix
 * array entries and interval bounds, :682-683,711-722,743-765); the environment variable QM_FORCE_BIGSA=1
 * writes that form for any text (tests).  Host only. */
int qm_build_index(const char* fasta_path, const char* out_dir, int32_t k, int32_t no_clip_poly_a,
                   int32_t keep_duplicates, int32_t n_threads, int32_t perfect_hash);
/* ... with `-s / --headerSep` (src/RapMapSAIndexer.cpp:833-835,868,588): the transcript's name is its header up to the first
 * of these characters (NULL: space or tab, the default) */
int qm_build_index_ex(const char* fasta_path, const char* out_dir, int32_t k, int32_t no_clip_poly_a,
                      int32_t keep_duplicates, int32_t n_threads, int32_t perfect_hash, const char* header_sep);

/* XXH64 as the index builder uses it: KmerKeyHasher (include/RapMapUtils.hpp:236-238: XXH64 of the key's 8 bytes, seed 0) places
 * the records of hash.bin so that the reference's spp::sparse_hash_map finds them after unserialize(); also the key of the
 * duplicate-transcript filter.  (Diagnostics: tests hold it against the reference's src/xxhash.c.) */
uint64_t qm_xxh64(const void* data, uint64_t len, uint64_t seed);

/* ---- equivalence classes on the device ---------------------------------------------------------------------------------
 * What a RapMap / Salmon-style caller does with a fragment's hit list: take the set of transcripts it maps to and add one to the
 * count of that set, its equivalence class (Salmon's eq_classes.txt).  A unit's LABEL is the ascending list of the DISTINCT
 * qm_hit.tid values of its hit list hits[hit_offsets[u] .. hit_offsets[u + 1]) -- hit lists are neither sorted nor free of
 * repeats (an orphan unit is the left mate's run followed by the right mate's, include/RapMapUtils.hpp:1257-1262; -f and -s may
 * repeat a transcript) --; a unit without hits contributes nothing.  A qm_eqc maps every label to the unsigned 64-bit number of
 * units (or sum of weights) that carried it; identity is the full label, never its hash.  No cap on the length of a list.
 * The batch is folded where it lies, in device memory: a run that wants classes brings a few megabytes to the host once instead
 * of 32 bytes per hit and batch.  A table is not thread-safe (one per context / host thread; merge with qm_eqc_add_labels). */
typedef struct qm_eqc qm_eqc;   /* a label -> count table in the device memory of ctx's GPU */
/* flags bits 8..15: keep only that many low bits of the 64-bit key (0 = all; tests: forces collisions) */
int qm_eqc_create(qm_ctx* ctx, int64_t expected_classes, uint32_t flags, qm_eqc** out);
int qm_eqc_destroy(qm_eqc* t);
int qm_eqc_clear(qm_eqc* t);
/* fold the result of ctx's last map call (what qm_result_device names), on ctx's stream, before anything can overwrite it.
 * QM_E_STATE without a result, QM_E_ARG when table and context are on different devices. */
int qm_eqc_add(qm_eqc* t, qm_ctx* ctx);
/* fold n lists of tids held in HOST memory, any order, duplicates allowed; weights NULL = 1 each.  The one merge primitive: a
 * table fetched from another context, device or rank is folded in with its counts as weights. */
int qm_eqc_add_labels(qm_eqc* t, int64_t n, const int64_t* offsets, const uint32_t* tids, const uint64_t* weights);
int qm_eqc_size(qm_eqc* t, int64_t* n_classes, int64_t* n_tids, uint64_t* total_count);
/* canonical order: labels ascending, compared lexicographically as uint32 sequences */
int qm_eqc_fetch(qm_eqc* t, int64_t* label_offsets /*[n_classes+1]*/, uint32_t* tids, uint64_t* counts);
/* since creation / the last clear: how often the table was rebuilt larger, published slots a probing unit found to hold another
 * label, units of more than 8 hits (labelled by the queue launch), probe launches; QM_EQC_STAT_LAST_FOLD_US: the last fold (qm_eqc_add, the
 * last part of qm_eqc_add_labels) from its first launch to its last read-back, in microseconds, by HIP events on its stream */
enum { QM_EQC_STAT_GROWTHS = 0, QM_EQC_STAT_COLLISION_PROBES = 1, QM_EQC_STAT_LONG_UNITS = 2, QM_EQC_STAT_ROUNDS = 3, QM_EQC_STAT_LAST_FOLD_US = 4 };
int qm_eqc_stat(const qm_eqc* t, int which, int64_t* value);

/* ---- abundance estimation on the device: the EM over an equivalence-class table --------------------------------------------
 * (No counterpart in the reference; consumer of qm_eqc.  The step every consumer of eq_classes.txt performs next.)  With classes c
 * of label L_c and count n_c, a positive effective length e_t per transcript and alpha_t the fragments assigned to t, one
 * iteration is, all in float64:
 *     w_t = alpha_t / e_t     d_c = sum of w_t over t in L_c     r_c = n_c / d_c (0 when d_c < DBL_MIN: the class is skipped)
 *     alpha'_t = w_t * (sum of r_c over the classes that contain t)
 * A class of one tid has d_c = w_t, so its term is n_c: it is added as it is (nothing when w_t < DBL_MIN) instead of being rounded
 * twice; a transcript that occurs in single-tid classes only holds exactly its count.
 * Two launches per iteration and no floating-point atomic: every sum is taken by one wavefront in an order that the table alone
 * fixes (class index = ascending slot index; a transcript's classes ascending), so a run is reproducible bit for bit.  No bias
 * models, no online phase, no truncation of small values at the end.  Not thread-safe (one per host thread).
 * The variational Bayes method (qm_quant_set_method) differs in w_t alone: w_t = E(alpha_t + p_t) / e_t with a prior p_t >= 0 per
 * transcript and E(x) = exp(digamma(x)), 0 for x < 1e-10 -- a function of this library's own (qm_quant_exp_digamma), defined
 * operation by operation in DESIGN.md section 4.13, so that a variational run is reproducible bit for bit as well. */
typedef struct qm_quant qm_quant;   /* the bipartite graph of a table and the current alpha, in the device memory of the table's GPU */
/* no counterpart in the reference; consumer of qm_eqc.  A SNAPSHOT of t: later folds into t (or its destruction) do not alter the
 * quant object, which runs on a stream of its own.  n_txps: transcripts (alpha has that many entries); a label that names a tid
 * >= n_txps fails the create with QM_E_ARG.  eff_len: n_txps positive finite numbers, NULL = 1.0 each (QM_E_ARG otherwise).  An
 * empty table is valid.  The start is the uniform default of qm_quant_set_start. */
int qm_quant_create(qm_eqc* t, int64_t n_txps, const double* eff_len, qm_quant** out);
/* no counterpart in the reference; consumer of qm_eqc.  alpha0: n_txps non-negative finite numbers (QM_E_ARG otherwise); NULL = the
 * uniform default: total / M for the M transcripts that occur in at least one label, 0 for all others (they stay 0). */
int qm_quant_set_start(qm_quant* q, const double* alpha0);
/* no counterpart in the reference; consumer of qm_eqc.  The method of every later qm_quant_run and of every qm_boot made later: the
 * EM (the default) or the variational Bayes EM with the prior p_t.  alpha stays as it is: a run begins with the weights of the
 * current alpha under its method, so a caller may run EM iterations and go on in VBEM.  What alpha reports does not change: the
 * expected fragments, without the prior.  An unknown method, or a prior that is negative or not finite: QM_E_ARG; while a qm_boot
 * borrows q: QM_E_STATE; nothing is changed then.  (Salmon's per-nucleotide prior is p_t = P * e_t, its per-transcript one
 * p_t = P; its default P is believed to be 1e-2.  Parity with Salmon is not claimed: none was at hand to compare with.) */
enum { QM_QUANT_METHOD_EM = 0, QM_QUANT_METHOD_VBEM = 1 };
int qm_quant_set_method(qm_quant* q, int method, const double* prior /*[n_txps] >= 0 and finite; NULL: 0.0 each; ignored for EM*/);
/* no counterpart in the reference.  E over an array: out[i] = E(x[i]), one small launch on `device`, for tests and callers */
int qm_quant_exp_digamma(int device, const double* x, int64_t n, double* out);
/* no counterpart in the reference; consumer of qm_eqc.  Up to max_iter iterations from the current alpha (a later call goes on
 * where the last one stopped).  Every check_every-th iteration (>= 1) the host reads one word: the largest |alpha'_t - alpha_t| /
 * alpha'_t over the transcripts with alpha'_t > min_alpha (>= 0); below rel_tol the run stops.  rel_tol = 0: exactly max_iter
 * iterations and no read-back at all.  Salmon's offline EM: max_iter 10000, check_every 10, rel_tol 1e-2, min_alpha 1e-8.
 * iterations: the iterations of this call; last_rel_change: the last value read, -1 when none was.  Either may be NULL. */
int qm_quant_run(qm_quant* q, int32_t max_iter, int32_t check_every, double rel_tol, double min_alpha, int32_t* iterations, double* last_rel_change);
/* no counterpart in the reference; consumer of qm_eqc.  The current alpha: n_txps doubles, all that crosses PCIe. */
int qm_quant_fetch(qm_quant* q, double* alpha /*[n_txps]*/);
/* no counterpart in the reference; consumer of qm_eqc.  Classes and label entries of the snapshot, transcripts that occur in a
 * label (M), the longest label and the longest transcript list, labels / transcript lists of more than 8 entries (handled one
 * per wavefront), the last qm_quant_run from its first launch to its last, and the structure build inside qm_quant_create (its
 * read-backs included), both in microseconds, by HIP events on its stream */
enum { QM_QUANT_STAT_CLASSES = 0, QM_QUANT_STAT_ENTRIES = 1, QM_QUANT_STAT_PRESENT = 2, QM_QUANT_STAT_LONGEST_LABEL = 3, QM_QUANT_STAT_LONGEST_LIST = 4,
       QM_QUANT_STAT_QUEUED_LABELS = 5, QM_QUANT_STAT_QUEUED_TXPS = 6, QM_QUANT_STAT_LAST_RUN_US = 7, QM_QUANT_STAT_BUILD_US = 8 };
int qm_quant_stat(const qm_quant* q, int which, int64_t* value);
/* no counterpart in the reference; consumer of qm_eqc */
int qm_quant_destroy(qm_quant* q);

/* ---- bootstrap replicates of the abundance estimate (Salmon's --numBootstraps) -------------------------
 * A replicate resamples the snapshot's class counts -- a multinomial over the classes, N = their sum draws -- and runs the EM of
 * qm_quant on the resampled counts; B replicates are iterated at once, every per-replicate array replicate-innermost, so that one
 * gathered item is a run of contiguous doubles.  The draw is defined exactly (n_c: the snapshot's counts in the order of
 * qm_quant_fetch_classes, cum their exclusive prefix sum; seed, R, k unsigned 64-bit): draw j (0 <= j < N) of replicate number R is
 *   k = j >> 1;  (x0, x1, x2, x3) = Philox4x32-10(counter = (lo k, hi k, lo R, hi R), key = (lo seed, hi seed));
 *   u = (j & 1) ? (x2 | x3 << 32) : (x0 | x1 << 32);  p = the high 64 bits of u * N;  the class c with cum[c] <= p < cum[c + 1]
 * so a replicate's counts depend on (snapshot, seed, R) alone, and its alpha on those and the run's arguments: not on n_reps, not
 * on its slot.  A resample costs N draws per replicate, whatever the number of classes.  Not thread-safe (one per host thread,
 * and not concurrently with its qm_quant: they share a stream). */
typedef struct qm_boot qm_boot;     /* the counts, weights and alphas of n_reps replicates over the graph of a qm_quant */
/* no counterpart in the reference; consumer of qm_quant.  The snapshot's class side in the snapshot's own order (ascending slot
 * index of the table it was taken from; NOT the sorted order of qm_eqc_fetch): offsets[classes + 1], tids[entries],
 * counts[classes] (QM_QUANT_STAT_CLASSES, _ENTRIES).  QM_E_UNSUPPORTED when the counts add up to 2^53 or more. */
int qm_quant_fetch_classes(qm_quant* q, int64_t* offsets /*[classes+1]*/, uint32_t* tids, uint64_t* counts);
/* no counterpart in the reference; consumer of qm_quant.  Borrows q's graph, effective lengths and stream: qm_quant_destroy(q)
 * returns QM_E_STATE and destroys nothing while a qm_boot of it lives.  n_reps < 1: QM_E_ARG; more than 65535: QM_E_UNSUPPORTED
 * (run batches: first_rep); no memory: QM_E_NOMEM with everything freed.  An empty table is valid. */
int qm_boot_create(qm_quant* q, int32_t n_reps, qm_boot** out);
/* no counterpart in the reference; consumer of qm_quant.  Slot i (0 <= i < n_reps) receives the counts of replicate number
 * first_rep + i under `seed`, its uniform start (N / M for the M transcripts that occur in a label) and starts anew: iteration
 * count, done flag. */
int qm_boot_resample(qm_boot* b, uint64_t seed, int64_t first_rep);
/* no counterpart in the reference; consumer of qm_quant.  One slot's counts as given (a resampling scheme of the caller's own),
 * in the order of qm_quant_fetch_classes; the slot starts anew from (their sum) / M.  rep outside [0, n_reps): QM_E_ARG. */
int qm_boot_set_counts(qm_boot* b, int32_t rep, const uint64_t* counts /*[classes]*/);
/* no counterpart in the reference; consumer of qm_quant.  One slot's counts. */
int qm_boot_fetch_counts(qm_boot* b, int32_t rep, uint64_t* counts /*[classes]*/);
/* no counterpart in the reference; consumer of qm_quant.  qm_quant_run's arguments and stopping rule, PER REPLICATE: on a checking
 * iteration every replicate's largest relative change is held against rel_tol; a replicate below it is done and frozen -- nothing
 * of it is written again, by this or a later call -- while the others go on; the host reads one word per check (how many are
 * done).  rel_tol = 0: exactly max_iter iterations, no read-back.  A later call goes on with the replicates that are not done.
 * iterations[i]: the iterations slot i made in this call; last_rel_change[i]: the last value held against rel_tol (-1: none yet;
 * a replicate done before this call keeps the value it stopped at).  Either may be NULL.  Before any qm_boot_resample or
 * qm_boot_set_counts: QM_E_STATE. */
int qm_boot_run(qm_boot* b, int32_t max_iter, int32_t check_every, double rel_tol, double min_alpha,
                int32_t* iterations /*[n_reps]*/, double* last_rel_change /*[n_reps]*/);
/* no counterpart in the reference; consumer of qm_quant.  The current alphas, transposed on the device and copied once. */
int qm_boot_fetch(qm_boot* b, double* alpha /*[n_reps][n_txps], row-major*/);
/* no counterpart in the reference; consumer of qm_quant.  Replicates; draws per replicate of the last resample (N); the last
 * resample and the last run in microseconds, by HIP events on the stream; kernel launches of the last run; labels / transcript
 * lists of more than 32 entries (one wavefront per row and tile of 16 replicates) */
enum { QM_BOOT_STAT_REPLICATES = 0, QM_BOOT_STAT_DRAWS = 1, QM_BOOT_STAT_LAST_RESAMPLE_US = 2, QM_BOOT_STAT_LAST_RUN_US = 3, QM_BOOT_STAT_LAUNCHES = 4,
       QM_BOOT_STAT_QUEUED_LABELS = 5, QM_BOOT_STAT_QUEUED_TXPS = 6 };
int qm_boot_stat(const qm_boot* b, int which, int64_t* value);
/* no counterpart in the reference; consumer of qm_quant */
int qm_boot_destroy(qm_boot* b);

/* ---- fragment-length distribution and effective lengths from the mapped pairs ---------------------------------------------
 * (No counterpart in the reference; consumer of the hit records.)  A qm_fld is a histogram fragment length -> number of fragments
 * in the device memory of a context's GPU: count[l], 0 <= l <= max_len, unsigned 64-bit; bin 0 exists and is never used.  A batch
 * is folded where it lies.  Every unit u of a batch falls into exactly one of six categories -- the first condition that holds --,
 * each with a 64-bit counter; the six always add up to the units folded:
 *     unmapped      hit_offsets[u + 1] - hit_offsets[u] == 0
 *     multi         ... >= 2
 *     not_paired    the one hit has mate_status != 3 (PE_PAIRED)
 *     same_strand   fwd == mate_is_fwd (where fragLengthPedantic answers 0)
 *     out_of_range  frag_len == 0 or frag_len > max_len, compared as unsigned 32-bit numbers (a wrapped negative lands here)
 *     used          otherwise: count[frag_len] += 1
 * The length is the record's frag_len as it stands (what pair_merge / unit_merge / sel_unit_merge set, as mergeLeftRightHits does,
 * include/RapMapUtils.hpp:1185-1264); it is NOT clipped to the transcript's end.  A single-end batch is valid: every mapped unit
 * is not_paired.  Integer adds only: a histogram does not depend on the grid or on the order the wavefronts arrive in.
 * Effective lengths, a defined model of this project (no prior, no smoothing; not Salmon's, and not held against it): with
 * P[m] = sum of count[l] and Q[m] = sum of l * count[l] over 1 <= l <= m, both 64-bit integers, a transcript of length L has,
 * with m = min(L, max_len),
 *     e = (double)L                                          when P[m] == 0
 *     e = (double)(L + 1) - (double)Q[m] / (double)P[m]      otherwise (one division, one subtraction, nothing fused)
 * -- the length minus the mean of the fragment lengths that fit, plus one; e >= 1 without a clamp.  A caller who wants a prior
 * adds pseudo-counts (qm_fld_add_counts).  Not thread-safe (one per context / host thread; merge with qm_fld_add_counts). */
typedef struct qm_fld qm_fld;
#define QM_FLD_DEFAULT_MAX_LEN 1000
/* no counterpart in the reference; consumer of the hit records.  1 <= max_len <= 1023 (max_len + 1 bins of 4 bytes are one 4 KB
 * slab per wavefront): 0 or negative is QM_E_ARG, above 1023 QM_E_UNSUPPORTED.  flags & 0xffff: at most that many workgroups per
 * fold (0 = as many as are resident; tests, tuning); other bits must be 0. */
int qm_fld_create(qm_ctx* ctx, int32_t max_len, uint32_t flags, qm_fld** out);
/* no counterpart in the reference; consumer of the hit records */
int qm_fld_destroy(qm_fld* f);
/* no counterpart in the reference; consumer of the hit records.  Bins and counters back to zero. */
int qm_fld_clear(qm_fld* f);
/* no counterpart in the reference; consumer of the hit records.  Folds the result of ctx's last map call (what qm_result_device
 * names) where it lies, on ctx's stream, before anything can overwrite it.  QM_E_STATE without a result, QM_E_ARG when histogram
 * and context are on different devices. */
int qm_fld_add(qm_fld* f, qm_ctx* ctx);
/* no counterpart in the reference; consumer of the hit records.  The same kernel over arrays in HOST memory, uploaded in parts.
 * hits may be NULL when no unit has a hit. */
int qm_fld_add_hits(qm_fld* f, int64_t n_units, const int64_t* hit_offsets, const qm_hit* hits);
/* no counterpart in the reference; consumer of the hit records.  count[l] += counts[l]: the merge primitive (contexts, devices,
 * ranks) and the way to a prior.  Their sum is added to `used` and to the units.  counts[0] != 0: QM_E_ARG. */
int qm_fld_add_counts(qm_fld* f, const uint64_t* counts /*[max_len+1]*/);
/* no counterpart in the reference; consumer of the hit records */
int qm_fld_fetch(qm_fld* f, uint64_t* counts /*[max_len+1]*/);
/* no counterpart in the reference; consumer of the hit records.  Since creation / the last clear: the units folded, the six
 * categories, max_len, the folds, and the last fold's kernel in microseconds, by HIP events on the fold's stream */
enum { QM_FLD_STAT_UNITS = 0, QM_FLD_STAT_USED = 1, QM_FLD_STAT_UNMAPPED = 2, QM_FLD_STAT_MULTI = 3, QM_FLD_STAT_NOT_PAIRED = 4, QM_FLD_STAT_SAME_STRAND = 5,
       QM_FLD_STAT_OUT_OF_RANGE = 6, QM_FLD_STAT_MAX_LEN = 7, QM_FLD_STAT_FOLDS = 8, QM_FLD_STAT_LAST_FOLD_US = 9 };
int qm_fld_stat(const qm_fld* f, int which, int64_t* value);
/* no counterpart in the reference; consumer of the hit records.  The arithmetic above as a pure host function: no device, no
 * context.  lens[i] == 0, counts[0] != 0, max_len < 1: QM_E_ARG; max_len > 1023, or Q[max_len] reaching 2^53: QM_E_UNSUPPORTED. */
int qm_fld_eff_lens_from_counts(int32_t max_len, const uint64_t* counts /*[max_len+1]*/, int64_t n_txps, const uint32_t* lens, double* eff /*[n_txps]*/);
/* no counterpart in the reference; consumer of the hit records.  qm_fld_fetch + qm_fld_eff_lens_from_counts. */
int qm_fld_eff_lens(qm_fld* f, int64_t n_txps, const uint32_t* lens, double* eff /*[n_txps]*/);

/* ---- fragment GC bias: observed and expected fragment GC, effective lengths -------------------------------------------------
 * (No counterpart in the reference; consumer of the hit records and of the transcript text.  The names follow Salmon's --gcBias;
 * parity with Salmon is NOT claimed: none was at hand to compare with.  QM_GCB_BINS and the ratio clamp of 1000 are constants of
 * this model.)  Integers only, except the closing host arithmetic.
 *   GC of a character: 1 for G, C, g, c, else 0.  GC_t(s, e): the sum over characters s .. e - 1 of transcript t.
 *   Bin of a window of n >= 1 characters holding g GC characters: min(QM_GCB_BINS - 1, (g * QM_GCB_BINS) / n), integer division.
 * OBSERVED: obs[QM_GCB_BINS], unsigned 64-bit.  Every unit of a batch falls into exactly one of seven categories -- the first
 * condition that holds --, each with a 64-bit counter; the seven always add up to the units swept.  The first five are qm_fld's,
 * with the same conditions (unmapped, multi, not_paired, same_strand, out_of_range: frag_len == 0 or > max_len).  Then, with
 * s = min(max(pos, 0), max(mate_pos, 0)) (the start mergeLeftRightHits uses for fragLen, include/RapMapUtils.hpp:1135-1141) and
 * e = s + frag_len:
 *     overhang      tid >= n_txps or e > txpLen[tid]
 *     used          otherwise: obs[bin(GC_tid(s, e), frag_len)] += 1
 * EXPECTED: H[n_txps][QM_GCB_BINS], unsigned 64-bit, from a fragment-length histogram counts[0 .. max_len] (qm_fld's shape,
 * counts[0] == 0): with n_t(l, b) = #{ s in [0, L_t - l] : bin(GC_t(s, s + l), l) == b },
 *     H[t][b] = sum over l = 1 .. min(L_t, max_len) of counts[l] * n_t(l, b)
 * exact and order-free; sum over b of H[t][b] == (L_t + 1) * P[m] - Q[m], m = min(L_t, max_len), P and Q as in qm_fld above.
 * EFFECTIVE LENGTHS, float64, every operation on its own (nothing fused), sums in ascending order of their index:
 *     S_t      = sum over b of H[t][b] (integer);   M_t = P[min(L_t, max_len)]
 *     exp[b]   = sum over t with alpha_t > 0 and S_t > 0 of alpha_t * ((double)H[t][b] / (double)S_t)
 *     O        = sum over b of obs[b] (integer);   E = sum over b of exp[b]
 *     ratio[b] = 1.0 when O == 0, E == 0 or exp[b] == 0; else ((double)obs[b] / (double)O) / (exp[b] / E), clamped to [1e-3, 1e3]
 *     e'_t     = (double)L_t when M_t == 0; else (sum over b of ratio[b] * (double)H[t][b]) / (double)M_t
 * With ratio == 1 this is S_t / M_t, qm_fld's effective length as one quotient.
 * The GC rank structure (a 64-bit mask per 64 text characters and the GC characters in front of each block, 12 bytes per 64
 * characters) lives in the index replica of the device and is built by the first qm_gcb_create of any context on it.
 * Not thread-safe (one per context / host thread; merge with qm_gcb_add_counts). */
typedef struct qm_gcb qm_gcb;
#define QM_GCB_BINS 25
/* no counterpart in the reference.  1 <= max_len <= 1023: 0 or negative is QM_E_ARG, above 1023 QM_E_UNSUPPORTED.
 * flags & 0xffff: at most that many workgroups per launch (0 = as many as are resident; tests, tuning); other bits must be 0. */
int qm_gcb_create(qm_ctx* ctx, int32_t max_len, uint32_t flags, qm_gcb** out);
/* no counterpart in the reference */
int qm_gcb_destroy(qm_gcb* g);
/* no counterpart in the reference.  Bins and counters back to zero. */
int qm_gcb_clear(qm_gcb* g);
/* no counterpart in the reference.  Sweeps the result of ctx's last map call where it lies, on ctx's stream, before anything can
 * overwrite it.  QM_E_STATE without a result, QM_E_ARG when object and context are on different devices or indexes. */
int qm_gcb_add(qm_gcb* g, qm_ctx* ctx);
/* no counterpart in the reference.  The same kernel over arrays in HOST memory, uploaded in parts.  hits may be NULL when no
 * unit has a hit. */
int qm_gcb_add_hits(qm_gcb* g, int64_t n_units, const int64_t* hit_offsets, const qm_hit* hits);
/* no counterpart in the reference.  obs[b] += counts[b]: the merge primitive (contexts, devices, ranks).  Their sum is added to
 * `used` and to the units. */
int qm_gcb_add_counts(qm_gcb* g, const uint64_t* obs /*[QM_GCB_BINS]*/);
/* no counterpart in the reference */
int qm_gcb_fetch(qm_gcb* g, uint64_t* obs /*[QM_GCB_BINS]*/);
/* no counterpart in the reference.  Since creation / the last clear: the units swept, the seven categories, max_len, the folds,
 * the last fold's kernel and the last qm_gcb_expect's kernel in microseconds (HIP events), and the microseconds this object spent
 * building the replica's rank structure (0 when it was there already; not cleared) */
enum { QM_GCB_STAT_UNITS = 0, QM_GCB_STAT_USED = 1, QM_GCB_STAT_UNMAPPED = 2, QM_GCB_STAT_MULTI = 3, QM_GCB_STAT_NOT_PAIRED = 4, QM_GCB_STAT_SAME_STRAND = 5,
       QM_GCB_STAT_OUT_OF_RANGE = 6, QM_GCB_STAT_OVERHANG = 7, QM_GCB_STAT_MAX_LEN = 8, QM_GCB_STAT_FOLDS = 9, QM_GCB_STAT_LAST_FOLD_US = 10,
       QM_GCB_STAT_LAST_EXPECT_US = 11, QM_GCB_STAT_RANK_BUILD_US = 12 };
int qm_gcb_stat(const qm_gcb* g, int which, int64_t* value);
/* no counterpart in the reference.  The expected matrix H[n_txps][QM_GCB_BINS] of counts[0 .. max_len] over every transcript of
 * the index (n_txps must be the index's).  counts[0] != 0: QM_E_ARG; P[max_len] * (the longest transcript) >= 2^63:
 * QM_E_UNSUPPORTED. */
int qm_gcb_expect(qm_gcb* g, const uint64_t* counts /*[max_len+1]*/, int64_t n_txps, uint64_t* H /*[n_txps*QM_GCB_BINS]*/);
/* no counterpart in the reference.  The arithmetic above as a pure host function: no device, no context.  exp_out and ratio_out
 * (QM_GCB_BINS doubles each) may be NULL.  lens[i] == 0, counts[0] != 0, max_len < 1: QM_E_ARG; max_len > 1023: QM_E_UNSUPPORTED. */
int qm_gcb_eff_lens_from_counts(int32_t max_len, const uint64_t* counts /*[max_len+1]*/, int64_t n_txps, const uint32_t* lens,
                                const uint64_t* H /*[n_txps*QM_GCB_BINS]*/, const double* alpha /*[n_txps]*/, const uint64_t* obs /*[QM_GCB_BINS]*/,
                                double* eff /*[n_txps]*/, double* exp_out, double* ratio_out);
/* no counterpart in the reference.  A probe of the rank structure: out[i] = GC_tids[i](starts[i], starts[i] + lens[i]), or -1
 * where the window is empty or does not lie on the transcript. */
int qm_gcb_window_gc(qm_gcb* g, int64_t n, const uint32_t* tids, const int32_t* starts, const int32_t* lens, int32_t* out /*[n]*/);

/* ---- sequence-specific bias: the nucleotide contexts at the two ends of a fragment ------------------------------------------
 * (No counterpart in the reference; consumer of the hit records and of the transcript text.  The names follow Salmon's --seqBias;
 * parity with Salmon is NOT claimed: none was at hand to compare with.  The model is this project's own and every constant in it
 * -- the context of 9 with 3 upstream, the order 2, the pseudo-count 1, the clamp [0.25, 4], the exponent 61 -- is a constant of
 * this model.)
 * CODES: A, a = 0; C, c = 1; G, g = 2; T, t = 3; any other byte is AMBIGUOUS.
 * CONTEXTS: a fragment lies on transcript t of length L as [s, e), e = s + frag_len, s = min(max(pos, 0), max(mate_pos, 0)) as
 * in the GC model above.  QM_SQB_CTX = 9 characters, QM_SQB_UP = 3 of them upstream of the end.
 *     5' context of start s:              c_j = code(t[s - 3 + j]), j = 0 .. 8; it lies on the transcript when 3 <= s <= L - 6
 *     3' context of last position i = e - 1 (the reverse strand): c_j = 3 - code(t[i + 3 - j]); when 5 <= i <= L - 4
 * and a context is VALID when it lies on the transcript and none of its nine characters is ambiguous.
 * WORDS (a position-specific model of order 2; every word is below 64):
 *     w_0 = c_0;   w_1 = 4 c_0 + c_1;   w_j = 16 c_(j-2) + 4 c_(j-1) + c_j for j >= 2
 * A table is [2 ends][QM_SQB_CTX][64] = QM_SQB_BINS = 1152 entries, end 0 the 5' end; entry (end, j, w) is at (end * 9 + j) * 64 + w.
 * OBSERVED: obs[QM_SQB_BINS], unsigned 64-bit.  Every unit of a batch falls into exactly one of eight categories -- the first
 * condition that holds --, each with a 64-bit counter; the eight always add up to the units swept.  The first five are qm_fld's
 * (unmapped, multi, not_paired, same_strand, out_of_range).  Then
 *     overhang      tid >= n_txps, or e > L, or one of the two contexts does not lie on the transcript
 *     ambiguous     one of the two contexts holds an ambiguous character
 *     used          otherwise: obs[end][j][w_j] += 1 for the nine words of each end (18 increments)
 * WEIGHTS (qm_sqb_weights, a pure host function; float64 under fp contract(off), every operation on its own): from a first
 * estimate alpha, the transcript lengths and a fragment-length histogram counts[0 .. m] (qm_fld's shape, counts[0] == 0), with
 * P[d] = sum of counts[l] over l <= d and Q[d] = sum of l * counts[l], both integers:
 *     S_t   = (L_t + 1) * P[m'] - Q[m'], m' = min(L_t, m): the (start, length) placements on t, an integer
 *     rho_t = alpha_t / (double)S_t; 0 when alpha_t > 0 does not hold or S_t == 0
 *     X     = sum over t ascending of rho_t * (double)L_t (a product and an addition each)
 *     k     = 61 - ilogb(X * (double)P[m]);  q_t = (uint64) floor(ldexp(rho_t, k))
 * When X * (double)P[m] is 0, k = 0 and every q_t = 0; when it is not finite: QM_E_ARG.  The rule keeps
 * sum of q_t * L_t * P[m] below 2^62 (1 + T 2^-52) < 2^63, which is what the expected counts need.
 * EXPECTED: exp[QM_SQB_BINS], unsigned 64-bit, on the device, integers only, hence order-free:
 *     exp[0][j][w] = sum over t of q_t * sum over the valid 5' contexts of t, at start s, of P[min(m, L_t - s)] * [w_j == w]
 *     exp[1][j][w] = sum over t of q_t * sum over the valid 3' contexts of t, at last position i, of P[min(m, i + 1)] * [w_j == w]
 * -- P[min(m, L_t - s)]: the fragments that may start at s; P[min(m, i + 1)]: those that may end at i.  THE TWO ENDS ARE COUNTED
 * INDEPENDENTLY: a start is not asked for a valid end and an end not for a valid start, while `used` needs both; the ratios below
 * are taken within an end, so a common factor between the ends does not reach them.  For each end the sum over w of exp[end][j][w]
 * is the same for all nine j.  sum of q_t * L_t * P[m] >= 2^63 (128-bit host arithmetic): QM_E_UNSUPPORTED.
 * RATIOS (qm_sqb_ratios, a pure host function): per end, position j and group of the four words that share w >> 2 (the same
 * two characters in front):
 *     po = (double)(obs + 1) / (double)(sum of the group's obs + 4);   pe likewise from exp;   R = min(max(po / pe, 0.25), 4.0)
 * Entries no context can produce (j = 0: w >= 4; j = 1: w >= 16) hold 1.0.
 * EFFECTIVE LENGTHS, on the device, float64, nothing fused:
 *     b5_t(s) = ((...((1.0 * R[0][0][w_0]) * R[0][1][w_1]) ...) * R[0][8][w_8]) for a valid 5' context at s, 1.0 otherwise
 *     b3_t(i) the same over R[1] for the 3' context at last position i
 *     N_t     = sum over l = 1 .. min(m, L_t) of counts[l] * sum over s = 0 .. L_t - l of b5(s) * b3(s + l - 1)
 *     e'_t    = N_t / (double)P[min(L_t, m)]; (double)L_t when that P is 0
 * in this order: per start s, a_s = the sum over ascending l (those with counts[l] != 0 and l <= min(m, L_t - s)) of
 * (double)counts[l] * b3(s + l - 1), starting from 0.0, one product and one addition each; v_s = b5(s) * a_s; the v of 64
 * consecutive starts 64 k .. 64 k + 63 (a tile; an absent start counts 0.0) are added by the tree
 *     rows of 16: x0..x15 -> ((x0 + x1) + (x2 + x3)) + ((x4 + x5) + (x6 + x7)), plus the same over x8..x15; then (R0 + R1) + (R2 + R3)
 * and a transcript's tiles are added in ascending order, starting from 0.0.  With R == 1 every term is an integer: N_t = S_t
 * exactly while S_t < 2^53, and e' is qm_fld's effective length as one quotient.
 * Not thread-safe (one per context / host thread; merge with qm_sqb_add_counts). */
typedef struct qm_sqb qm_sqb;
#define QM_SQB_CTX 9
#define QM_SQB_UP 3
#define QM_SQB_BINS 1152
/* no counterpart in the reference.  max_len and flags as qm_gcb_create's. */
int qm_sqb_create(qm_ctx* ctx, int32_t max_len, uint32_t flags, qm_sqb** out);
/* no counterpart in the reference */
int qm_sqb_destroy(qm_sqb* g);
/* no counterpart in the reference.  Observed counts and counters back to zero. */
int qm_sqb_clear(qm_sqb* g);
/* no counterpart in the reference.  Sweeps the result of ctx's last map call where it lies, as qm_gcb_add does. */
int qm_sqb_add(qm_sqb* g, qm_ctx* ctx);
/* no counterpart in the reference.  The same kernel over arrays in HOST memory, uploaded in parts. */
int qm_sqb_add_hits(qm_sqb* g, int64_t n_units, const int64_t* hit_offsets, const qm_hit* hits);
/* no counterpart in the reference.  obs[i] += counts[i]: the merge primitive.  A used fragment brings 18 counts, one of them at (end 0,
 * j = 0): the sum of counts[0][0][.] is added to `used` and to the units. */
int qm_sqb_add_counts(qm_sqb* g, const uint64_t* obs /*[QM_SQB_BINS]*/);
/* no counterpart in the reference */
int qm_sqb_fetch(qm_sqb* g, uint64_t* obs /*[QM_SQB_BINS]*/);
/* no counterpart in the reference.  Since creation / the last clear: the units swept, the eight categories, max_len, the folds and
 * the kernels of the last fold, the last qm_sqb_expect and the last qm_sqb_eff_lens in microseconds (HIP events) */
enum { QM_SQB_STAT_UNITS = 0, QM_SQB_STAT_USED = 1, QM_SQB_STAT_UNMAPPED = 2, QM_SQB_STAT_MULTI = 3, QM_SQB_STAT_NOT_PAIRED = 4, QM_SQB_STAT_SAME_STRAND = 5,
       QM_SQB_STAT_OUT_OF_RANGE = 6, QM_SQB_STAT_OVERHANG = 7, QM_SQB_STAT_AMBIGUOUS = 8, QM_SQB_STAT_MAX_LEN = 9, QM_SQB_STAT_FOLDS = 10,
       QM_SQB_STAT_LAST_FOLD_US = 11, QM_SQB_STAT_LAST_EXPECT_US = 12, QM_SQB_STAT_LAST_EFFLEN_US = 13 };
int qm_sqb_stat(const qm_sqb* g, int which, int64_t* value);
/* no counterpart in the reference.  exp[QM_SQB_BINS] from counts[0 .. max_len] and the weights q[n_txps] over every transcript of
 * the index (n_txps must be the index's).  counts[0] != 0: QM_E_ARG; 2^63 fragments or more, or the bound above: QM_E_UNSUPPORTED. */
int qm_sqb_expect(qm_sqb* g, const uint64_t* counts /*[max_len+1]*/, int64_t n_txps, const uint64_t* q /*[n_txps]*/, uint64_t* exp /*[QM_SQB_BINS]*/);
/* no counterpart in the reference.  eff[n_txps] from counts[0 .. max_len] and the ratios R[QM_SQB_BINS].  counts[0] != 0: QM_E_ARG. */
int qm_sqb_eff_lens(qm_sqb* g, const uint64_t* counts /*[max_len+1]*/, int64_t n_txps, const double* R /*[QM_SQB_BINS]*/, double* eff /*[n_txps]*/);
/* no counterpart in the reference.  A probe of the contexts: question i asks for the context of end ends[i] (0: 5', 1: 3') at
 * position positions[i] (the start s, or the last position i) of transcript tids[i]; out[9 i .. 9 i + 8] are its nine words, or
 * all -1 where the context is not valid. */
int qm_sqb_context(qm_sqb* g, int64_t n, const uint32_t* tids, const int32_t* positions, const int32_t* ends, int32_t* out /*[n*9]*/);
/* no counterpart in the reference.  The weights above as a pure host function: q[n_txps] and the exponent k.  lens[i] == 0,
 * counts[0] != 0, max_len < 1, X * P[m] not finite: QM_E_ARG; max_len > 1023, 2^63 fragments or more, or (the longest transcript
 * + 1) * P[m] >= 2^63: QM_E_UNSUPPORTED. */
int qm_sqb_weights(int32_t max_len, const uint64_t* counts /*[max_len+1]*/, int64_t n_txps, const uint32_t* lens, const double* alpha /*[n_txps]*/,
                   uint64_t* q /*[n_txps]*/, int32_t* k);
/* no counterpart in the reference.  The ratios above as a pure host function. */
int qm_sqb_ratios(const uint64_t* obs /*[QM_SQB_BINS]*/, const uint64_t* exp /*[QM_SQB_BINS]*/, double* R /*[QM_SQB_BINS]*/);

/* ---- positional bias: where along its transcript a fragment starts and where it ends ---------------------------------------------
 * (No counterpart in the reference; consumer of the hit records.  The names follow Salmon's --posBias; parity with Salmon is NOT
 * claimed: none was at hand to compare with.  The model is this project's own and every constant in it -- the five length classes
 * and their bounds, the 20 bins, the pseudo-count 1, the clamp [0.25, 4] -- is a constant of this model.)
 * FRAGMENT: a fragment lies on transcript t of length L as [s, e), e = s + frag_len, s = min(max(pos, 0), max(mate_pos, 0)) as in
 * the GC model above; its last position is i = e - 1.  Everything is in transcript coordinates, as in the sequence model.
 * CLASSES: QM_PSB_CLASSES = 5, by transcript length: class 0: L <= 791; 1: L <= 1265; 2: L <= 1707; 3: L <= 2433; 4: otherwise.
 * BINS: QM_PSB_POS = 20.  Position x (0 <= x < L) falls in bin floor(20 x / L), exact integer arithmetic; equivalently bin b holds
 * [B_b, B_(b+1)) with B_b = ceil(b L / 20).  A transcript shorter than 20 has empty bins.
 * TABLE: [2 ends][5][20] = QM_PSB_BINS = 200 entries; entry (end, c, b) is at (end * 5 + c) * 20 + b.  End 0 is the start s, end 1
 * the last position i.
 * OBSERVED: obs[QM_PSB_BINS], unsigned 64-bit.  A unit falls into the first of seven categories that holds, each with a 64-bit
 * counter; the seven always add up to the units swept.  The first five are qm_fld's (unmapped, multi, not_paired, same_strand,
 * out_of_range).  Then
 *     overhang      tid >= n_txps, or e > L
 *     used          otherwise: obs[0][c][bin(s)] += 1 and obs[1][c][bin(i)] += 1, c the class of L
 * WEIGHTS: qm_sqb_weights as it is (q_t and k); this model adds no function of its own.
 * EXPECTED: exp[QM_PSB_BINS], unsigned 64-bit, on the device, integers only, hence order-free.  With P of the sequence model,
 * W[0] = 0 and W[x] = W[x - 1] + P[min(m, x)] -- so W[x] = W[m] + (x - m) P[m] beyond m, and W[L_t] = S_t.  A start s carries
 * P[min(m, L - s)], a last position i carries P[min(m, i + 1)]; summed over the positions of a bin:
 *     exp[0][c_t][b] += q_t * (W[L_t - B_b] - W[L_t - B_(b+1)])
 *     exp[1][c_t][b] += q_t * (W[B_(b+1)] - W[B_b])
 * a closed form per (transcript, bin).  Each end sums to the sum over t of q_t * S_t.  sum of q_t * L_t * P[m] >= 2^63 (128-bit
 * host arithmetic): QM_E_UNSUPPORTED, as in qm_sqb_expect.
 * RATIOS (qm_psb_ratios, a pure host function; float64 under fp contract(off), every operation on its own): per (end, class), over
 * its 20 bins,
 *     po = (double)(obs + 1) / (double)(sum of the 20 obs + 20);   pe likewise from exp;   R = min(max(po / pe, 0.25), 4.0)
 * and an (end, class) whose sum of obs or sum of exp is 0 holds 1.0 throughout.
 * EFFECTIVE LENGTHS, on the device, float64, nothing fused: the sequence model's definition with
 *     b5_t(s) = R[0][c_t][bin_t(s)]        b3_t(i) = R[1][c_t][bin_t(i)]
 * and everything else as it stands there: N_t; e'_t = N_t / (double)P[min(L_t, m)], (double)L_t where that P is 0; the order -- per
 * start ascending l, one product and one addition each, never fused; 64 starts by the tree; a transcript's tiles ascending.  With
 * R == 1 it is qm_fld's effective length as one quotient, bit for bit.
 * Not thread-safe (one per context / host thread; merge with qm_psb_add_counts). */
typedef struct qm_psb qm_psb;
#define QM_PSB_CLASSES 5
#define QM_PSB_POS 20
#define QM_PSB_BINS 200
/* no counterpart in the reference.  max_len and flags as qm_gcb_create's. */
int qm_psb_create(qm_ctx* ctx, int32_t max_len, uint32_t flags, qm_psb** out);
/* no counterpart in the reference */
int qm_psb_destroy(qm_psb* g);
/* no counterpart in the reference.  Observed counts and counters back to zero. */
int qm_psb_clear(qm_psb* g);
/* no counterpart in the reference.  Sweeps the result of ctx's last map call where it lies, as qm_gcb_add does. */
int qm_psb_add(qm_psb* g, qm_ctx* ctx);
/* no counterpart in the reference.  The same kernel over arrays in HOST memory, uploaded in parts. */
int qm_psb_add_hits(qm_psb* g, int64_t n_units, const int64_t* hit_offsets, const qm_hit* hits);
/* no counterpart in the reference.  obs[i] += counts[i]: the merge primitive.  A used fragment brings two counts, one of them at
 * end 0: the sum of counts[0][.][.] is added to `used` and to the units. */
int qm_psb_add_counts(qm_psb* g, const uint64_t* obs /*[QM_PSB_BINS]*/);
/* no counterpart in the reference */
int qm_psb_fetch(qm_psb* g, uint64_t* obs /*[QM_PSB_BINS]*/);
/* no counterpart in the reference.  Since creation / the last clear: the units swept, the seven categories, max_len, the folds and
 * the kernels of the last fold, the last qm_psb_expect and the last qm_psb_eff_lens in microseconds (HIP events) */
enum { QM_PSB_STAT_UNITS = 0, QM_PSB_STAT_USED = 1, QM_PSB_STAT_UNMAPPED = 2, QM_PSB_STAT_MULTI = 3, QM_PSB_STAT_NOT_PAIRED = 4, QM_PSB_STAT_SAME_STRAND = 5,
       QM_PSB_STAT_OUT_OF_RANGE = 6, QM_PSB_STAT_OVERHANG = 7, QM_PSB_STAT_MAX_LEN = 8, QM_PSB_STAT_FOLDS = 9, QM_PSB_STAT_LAST_FOLD_US = 10,
       QM_PSB_STAT_LAST_EXPECT_US = 11, QM_PSB_STAT_LAST_EFFLEN_US = 12 };
int qm_psb_stat(const qm_psb* g, int which, int64_t* value);
/* no counterpart in the reference.  exp[QM_PSB_BINS] from counts[0 .. max_len] and the weights q[n_txps] (qm_sqb_weights) over every
 * transcript of the index (n_txps must be the index's).  counts[0] != 0: QM_E_ARG; 2^63 fragments or more, or the bound above:
 * QM_E_UNSUPPORTED. */
int qm_psb_expect(qm_psb* g, const uint64_t* counts /*[max_len+1]*/, int64_t n_txps, const uint64_t* q /*[n_txps]*/, uint64_t* exp /*[QM_PSB_BINS]*/);
/* no counterpart in the reference.  eff[n_txps] from counts[0 .. max_len] and the ratios R[QM_PSB_BINS].  counts[0] != 0: QM_E_ARG. */
int qm_psb_eff_lens(qm_psb* g, const uint64_t* counts /*[max_len+1]*/, int64_t n_txps, const double* R /*[QM_PSB_BINS]*/, double* eff /*[n_txps]*/);
/* no counterpart in the reference.  A probe of classes and bins: question i asks for position positions[i] of transcript tids[i];
 * out[2 i] is the transcript's class and out[2 i + 1] the position's bin, or both -1 where tids[i] is no transcript of the index or
 * positions[i] no position of it. */
int qm_psb_position(qm_psb* g, int64_t n, const uint32_t* tids, const int32_t* positions, int32_t* out /*[n*2]*/);
/* no counterpart in the reference.  The ratios above as a pure host function. */
int qm_psb_ratios(const uint64_t* obs /*[QM_PSB_BINS]*/, const uint64_t* exp /*[QM_PSB_BINS]*/, double* R /*[QM_PSB_BINS]*/);

/* ---- library type: hit orientations tallied, compatible hits kept ------------------------------------------------------------
 * (No counterpart in the reference; consumer of the hit records.  The names follow Salmon's -l / --libType and its
 * lib_format_counts.json; parity with Salmon is NOT claimed: none was at hand to compare with.  The model is this project's own,
 * exactly defined, integers only.)  Every hit record has a CODE; a byte counts as forward when it is not 0:
 *     mate_status 3 (PE_PAIRED)   fwd != mate_is_fwd, not outward:  fwd 0 ISF, !fwd 1 ISR
 *                                 fwd != mate_is_fwd, outward:      fwd 2 OSF, !fwd 3 OSR
 *                                 both forward 4 MSF, both reverse 5 MSR
 *     mate_status 1 (PE_LEFT)     fwd 6 LF, !fwd 7 LR
 *     mate_status 2 (PE_RIGHT)    fwd 8 RF, !fwd 9 RR
 *     mate_status 0 (SINGLE_END)  fwd 10 SF, !fwd 11 SR
 *     mate_status > 3             no code: tallied as `other`, never kept
 * Outward is the reference's own dovetail predicate, (fwd && pos > mate_pos) || (mate_is_fwd && mate_pos > pos), compared as signed
 * numbers (src/RapMapSAMapper.cpp:539-551 as the oracle restates it): a DOVETAILING pair counts as outward.
 * A library type is a 12-bit mask over the codes (qm_lib_type_mask): IU = ISF ISR LF LR RF RR, ISF = ISF LF RR, ISR = ISR LR RF;
 * OU / OSF / OSR and MU the same with the O / M codes, MSF = MSF LF RF, MSR = MSR LR RR; U = SF SR, SF, SR; A = all twelve
 * (nothing is dropped, the run only reports).  A qm_lib holds one mask and 32 unsigned 64-bit tallies in device memory:
 *     [0..11] hits by code   [12..23] units with exactly one hit, by that hit's code   [24] units   [25] units without hits
 *     [26] kept units: at least one hit whose code is in the mask   [27] dropped units: hits, but none in the mask
 *     [28] hits   [29] kept hits   [30] `other` hits   [31] 0
 * so that sum [0..11] + [30] == [28], [25] + [26] + [27] == [24], and [29] is the sum of [0..11] over the mask's codes.
 * A unit's FILTERED hit list is its hit list without the hits outside the mask, order kept; its class label is defined on that
 * list as above (equivalence classes); a dropped unit contributes nothing, like a unit without hits.  Integer adds only: a tally
 * does not depend on the grid.  Not thread-safe (one per context / host thread; merge with qm_lib_add_counts). */
typedef struct qm_lib qm_lib;
#define QM_LIB_ALL_CODES 0xfffu
/* no counterpart in the reference; consumer of the hit records.  mask: the codes kept, 1 .. 0xfff (0, or a bit above 11: QM_E_ARG).
 * flags & 0xffff: at most that many workgroups per sweep (0 = as many as are resident; tests, tuning); other bits must be 0. */
int qm_lib_create(qm_ctx* ctx, uint32_t mask, uint32_t flags, qm_lib** out);
/* no counterpart in the reference; consumer of the hit records */
int qm_lib_destroy(qm_lib* lib);
/* no counterpart in the reference; consumer of the hit records.  The tallies back to zero. */
int qm_lib_clear(qm_lib* lib);
/* no counterpart in the reference; consumer of the hit records.  Tallies the result of ctx's last map call (what qm_result_device
 * names) where it lies, on ctx's stream, before anything can overwrite it.  QM_E_STATE without a result, QM_E_ARG when object and
 * context are on different devices. */
int qm_lib_add(qm_lib* lib, qm_ctx* ctx);
/* no counterpart in the reference; consumer of the hit records.  The same sweep over arrays in HOST memory, uploaded in parts.
 * hits may be NULL (or empty) when no unit has a hit. */
int qm_lib_add_hits(qm_lib* lib, int64_t n_units, const int64_t* hit_offsets, const qm_hit* hits);
/* no counterpart in the reference; consumer of the hit records.  qm_lib_add_hits, and the filtered lists brought back:
 * new_offsets[n_units + 1] (new_offsets[0] = 0) and the kept hits' tids[new_offsets[n_units]] (room for as many as there are hits). */
int qm_lib_compact_hits(qm_lib* lib, int64_t n_units, const int64_t* hit_offsets, const qm_hit* hits, int64_t* new_offsets, uint32_t* tids);
/* no counterpart in the reference; consumer of the hit records.  tally[i] += counts[i], i < 31: the merge primitive (contexts,
 * devices, ranks).  counts[31] != 0: QM_E_ARG. */
int qm_lib_add_counts(qm_lib* lib, const uint64_t counts[32]);
/* no counterpart in the reference; consumer of the hit records */
int qm_lib_fetch(qm_lib* lib, uint64_t counts[32]);
/* no counterpart in the reference; consumer of the hit records.  Since creation / the last clear: the sweeps; the last sweep from
 * its first launch to its last, in microseconds, by HIP events on its stream; the mask */
enum { QM_LIB_STAT_SWEEPS = 0, QM_LIB_STAT_LAST_SWEEP_US = 1, QM_LIB_STAT_MASK = 2 };
int qm_lib_stat(const qm_lib* lib, int which, int64_t* value);
/* no counterpart in the reference; consumer of the hit records and of qm_eqc.  qm_eqc_add over the FILTERED hit lists of ctx's last
 * map call: sweep and tally (into lib), compact the kept hits' tids, fold those.  Under the all-codes mask nothing is compacted: it
 * tallies and runs qm_eqc_add's fold.  QM_E_STATE without a result, QM_E_ARG unless all three are on one device. */
int qm_eqc_add_lib(qm_eqc* t, qm_ctx* ctx, qm_lib* lib);
/* no counterpart in the reference.  Pure host functions: no device, no context.  The mask of a type name (IU ISF ISR OU OSF OSR MU
 * MSF MSR U SF SR A, upper case); an unknown name is QM_E_ARG. */
int qm_lib_type_mask(const char* name, uint32_t* mask);
/* no counterpart in the reference.  The expected type from the single-hit words [12..23], 64-bit integer arithmetic only: with
 * I = ISF + ISR, O = OSF + OSR, M = MSF + MSR, S = SF + SR the orientation is the largest (ties: the earlier in that order; all
 * zero: ""); within it, a the forward-sense and b the reverse-sense count, 10 a > 7 (a + b) gives ..SF, 10 a < 3 (a + b) gives
 * ..SR, anything else ..U (for S: SF, SR, U).  A count of 2^59 or more: QM_E_UNSUPPORTED. */
int qm_lib_infer(const uint64_t counts[32], char out[4]);

/* ---- host-side callers of the path -------------------------------------------
 * Read ingest: replaces fastx_parser::FastxParser<ReadPair|ReadSeq> (include/FastxParser.hpp:62-66,
 * src/FastxParser.cpp:229-328: one kseq producer thread, per-record std::strings).  FASTA/FASTQ, plain or
 * gzip'd; path2 == NULL for single-end.  qm_reader_next hands out up to max_units records as packed batches
 * in exactly the form qm_map_pairs / qm_map_reads take; the pointers stay valid until the next call.
 * n_units == 0 means end of input.  Qualities are dropped, as the reference's parser does. */
typedef struct qm_reader qm_reader;
int qm_reader_open(const char* path1, const char* path2, int32_t n_threads, qm_reader** out);
int qm_reader_next(qm_reader* r, int64_t max_units, int64_t* n_units, const char** seq1, const int64_t** off1,
                   const char** names1, const int64_t** name_off1, const char** seq2, const int64_t** off2,
                   const char** names2, const int64_t** name_off2);
void qm_reader_close(qm_reader* r);
const char* qm_io_last_error(void);

/* FASTA/FASTQ files -> mapped batches, pipelined (the ingest side of the path; replaces the single kseq
 * producer + per-record std::strings of src/FastxParser.cpp:229-328, and the worker threads of spawnProcessReadsThreads,
 * src/RapMapSAMapper.cpp:752-799).  `reader_threads` workers parse the files chunk-parallel (plain files are cut at byte
 * offsets with record resync; .gz files are inflated by one thread per file, pipelined with the parsers) and pack batches
 * straight into pinned host slots, several batches in flight, while four device contexts per device (QM_STREAM_CTX_PER_DEVICE) (sharing that device's
 * index replica) upload, map and download the previous ones; with several devices consecutive batches go to different
 * devices (the static sharding of SURVEY.md section 8e inside one process).  The caller drains the batches IN INPUT ORDER,
 * whichever device mapped them.  Everything a batch points to -- reads, names, hit offsets, hits -- is pinned memory owned by
 * the stream and stays valid until the next qm_stream_next call.  n_units == 0: end of input.  path2 == NULL: single-end.
 * Counters come per batch; a run's HitCounters are their sum. */
typedef struct qm_stream qm_stream;
typedef struct qm_stream_batch {
  int64_t n_units;
  const char* seq1; const int64_t* off1; const char* names1; const int64_t* name_off1;
  const char* seq2; const int64_t* off2; const char* names2; const int64_t* name_off2;
  const int64_t* hit_offsets; const qm_hit* hits; int64_t n_hits;
  qm_counters counters;
  double gpu_ms;
  int32_t device;  /* the device that mapped this batch */
  int32_t pad;
} qm_stream_batch;
int qm_stream_open(const qm_index* ix, int device_id, uint32_t ctx_flags, const qm_opts* opts, const char* path1, const char* path2,
                   int64_t batch_units, int32_t reader_threads, qm_stream** out);
/* ... on the devices devices[0..n_devices).  stream_flags: QM_STREAM_NO_NAMES -- read names are not kept (names* / name_off*
 * of the batches are NULL): for callers that only want hits. */
#define QM_STREAM_NO_NAMES 1u
/* QM_STREAM_EQ_CLASSES -- every map context owns a qm_eqc and folds each batch into it after mapping; qm_stream_eqc_finish merges
 * them.  QM_STREAM_NO_HITS (only together with QM_STREAM_EQ_CLASSES) -- the hits are not brought to the host: hit_offsets and
 * hits of a batch are NULL; n_hits, counters, gpu_ms and device stay as they are. */
#define QM_STREAM_EQ_CLASSES 2u
#define QM_STREAM_NO_HITS 4u
/* QM_STREAM_FLD -- every map context owns a qm_fld of QM_FLD_DEFAULT_MAX_LEN and folds each batch into it after mapping, on the
 * context's stream, before the batch's buffers are reused; with or without QM_STREAM_EQ_CLASSES (QM_STREAM_NO_HITS keeps its rule:
 * only together with QM_STREAM_EQ_CLASSES).  qm_stream_fld_fetch sums the contexts' histograms. */
#define QM_STREAM_FLD 8u
/* QM_STREAM_LIB -- every map context owns a qm_lib whose mask is bits 16..27 of stream_flags (0 there: all codes).  Together with
 * QM_STREAM_EQ_CLASSES each batch is folded through qm_eqc_add_lib (the classes hold compatible hits only), without it each batch
 * is tallied by qm_lib_add; qm_stream_lib_fetch sums the contexts' tallies.  A stream without the flag creates no qm_lib and
 * launches nothing of it. */
#define QM_STREAM_LIB 16u
#define QM_STREAM_LIB_MASK_SHIFT 16
/* QM_STREAM_GCB -- every map context owns a qm_gcb of QM_FLD_DEFAULT_MAX_LEN and sweeps each batch into it after mapping (after the
 * QM_STREAM_FLD fold, when there is one), on the context's stream, before the batch's buffers are reused; with or without the other
 * flags.  qm_stream_gcb_fetch sums the contexts' observed counts.  A stream without the flag creates no qm_gcb, builds no rank
 * structure and launches nothing of it. */
#define QM_STREAM_GCB 32u
/* QM_STREAM_SQB -- every map context owns a qm_sqb of QM_FLD_DEFAULT_MAX_LEN and sweeps each batch into it after mapping (after the
 * QM_STREAM_GCB sweep, when there is one), on the context's stream, before the batch's buffers are reused; with or without the other
 * flags.  qm_stream_sqb_fetch sums the contexts' observed counts.  A stream without the flag creates no qm_sqb and launches nothing
 * of it. */
#define QM_STREAM_SQB 64u
/* QM_STREAM_PSB -- every map context owns a qm_psb of QM_FLD_DEFAULT_MAX_LEN and sweeps each batch into it after mapping (after the
 * QM_STREAM_SQB sweep, when there is one), on the context's stream, before the batch's buffers are reused; with or without the other
 * flags.  qm_stream_psb_fetch sums the contexts' observed counts.  A stream without the flag creates no qm_psb and launches nothing
 * of it. */
#define QM_STREAM_PSB 128u
int qm_stream_open_ex(const qm_index* ix, const int32_t* devices, int32_t n_devices, uint32_t ctx_flags, const qm_opts* opts,
                      const char* path1, const char* path2, int64_t batch_units, int32_t reader_threads, uint32_t stream_flags,
                      qm_stream** out);
/* Pinning host memory is slow (about 5.5 GB/s on this platform, whatever the number of threads): a stream's slots -- a few hundred
 * MB -- cost as much as mapping millions of pairs.  qm_stream_reserve(bytes) pins a process-wide pool in the background and
 * returns at once; streams carve their slots out of it and hand them back when they close, so only the first reservation of a
 * process pays.  Call it as early as possible (the CLI does, before it uploads the index); 512 MB serve one single-device
 * stream of 2^18-pair batches of 2 x 100 bp reads.  Optional: without it a stream pins its own slots while it starts. */
int qm_stream_reserve(int64_t bytes);
int qm_stream_next(qm_stream* s, qm_stream_batch* batch);
/* Once qm_stream_next has returned the end of the input: merges the contexts' tables, across devices, into the first one (through
 * qm_eqc_add_labels) and reports its size; qm_stream_eqc_fetch then hands it out as qm_eqc_fetch does. */
int qm_stream_eqc_finish(qm_stream* s, int64_t* n_classes, int64_t* n_tids);
int qm_stream_eqc_fetch(qm_stream* s, int64_t* label_offsets, uint32_t* tids, uint64_t* counts);
/* No counterpart in the reference; consumer of the hit records.  Once qm_stream_next has returned the end of the input (where
 * qm_stream_eqc_finish is valid; QM_E_STATE otherwise, and for a stream opened without QM_STREAM_FLD): the contexts' histograms and
 * counters summed, across devices.  stats7: the units, then used, unmapped, multi, not_paired, same_strand, out_of_range. */
int qm_stream_fld_fetch(qm_stream* s, uint64_t* counts /*[QM_FLD_DEFAULT_MAX_LEN+1]*/, int64_t* stats7);
/* No counterpart in the reference; consumer of the hit records.  Once qm_stream_next has returned the end of the input (QM_E_STATE
 * before that, and for a stream opened without QM_STREAM_LIB): the contexts' tallies summed, across devices. */
int qm_stream_lib_fetch(qm_stream* s, uint64_t counts[32]);
/* No counterpart in the reference; consumer of the hit records.  Once qm_stream_next has returned the end of the input (QM_E_STATE
 * before that, and for a stream opened without QM_STREAM_GCB): the contexts' observed GC counts and counters summed, across devices.
 * stats8: the units, then used, unmapped, multi, not_paired, same_strand, out_of_range, overhang. */
int qm_stream_gcb_fetch(qm_stream* s, uint64_t* obs /*[QM_GCB_BINS]*/, int64_t* stats8);
/* No counterpart in the reference; consumer of the hit records.  Once qm_stream_next has returned the end of the input (QM_E_STATE
 * before that, and for a stream opened without QM_STREAM_SQB): the contexts' observed sequence-bias counts and counters summed,
 * across devices.  stats9: the units, then used, unmapped, multi, not_paired, same_strand, out_of_range, overhang, ambiguous. */
int qm_stream_sqb_fetch(qm_stream* s, uint64_t* obs /*[QM_SQB_BINS]*/, int64_t* stats9);
/* No counterpart in the reference; consumer of the hit records.  Once qm_stream_next has returned the end of the input (QM_E_STATE
 * before that, and for a stream opened without QM_STREAM_PSB): the contexts' observed positional-bias counts and counters summed,
 * across devices.  stats8: the units, then used, unmapped, multi, not_paired, same_strand, out_of_range, overhang. */
int qm_stream_psb_fetch(qm_stream* s, uint64_t* obs /*[QM_PSB_BINS]*/, int64_t* stats8);
void qm_stream_close(qm_stream* s);
/* seconds spent so far: [0] the ingest engine, open to its last batch packed (wall), [1] upload + kernels (summed over the
 * contexts), [2] download (summed), [3] the caller waiting in qm_stream_next, [4] qm_stream_open, [5] growing the pinned result
 * buffers ([1] and [2] do not hold the folds of a QM_STREAM_EQ_CLASSES stream: those are [13]); qm_stream_stats_ex(n <= 19) adds [6] open to the first batch packed, [7] parse tasks (CPU seconds over all workers),
 * [8] copy tasks, [9] inflate threads, [10] bytes parsed, [11] open to the last batch mapped and downloaded (wall), [12] batches that went
 * to the device 2-bit packed, [13] qm_eqc_add of the batches (summed over the contexts), [14] contexts that folded at least one batch,
 * [15] qm_fld_add of the batches of a QM_STREAM_FLD stream (seconds, summed over the contexts; not part of [1], [2] or [13]),
 * [16] qm_gcb_add of the batches of a QM_STREAM_GCB stream (seconds, summed over the contexts; not part of [1], [2], [13] or [15]),
 * [17] qm_sqb_add of the batches of a QM_STREAM_SQB stream (seconds, summed over the contexts; not part of the others),
 * [18] qm_psb_add of the batches of a QM_STREAM_PSB stream (seconds, summed over the contexts; not part of the others) */
int qm_stream_stats(qm_stream* s, double* out6);
int qm_stream_stats_ex(qm_stream* s, double* out, int32_t n);
const char* qm_stream_last_error(void);

/* SAM text of a mapped batch, byte for byte what `rapmap quasimap -o` writes: header = writeSAMHeader
 * (include/RapMapUtils.hpp:97-115); records = writeAlignmentsToStream / writeUnalignedPairToStream
 * (src/RapMapUtils.cpp:137-196,198-311,313-588) with getSamFlags / adjustOverhang
 * (include/RapMapUtils.hpp:687-810).  seq2 == NULL: single-end records.  The text is malloc'd; release it
 * with qm_buf_free. */
int qm_sam_header(const qm_index* ix, char** out, int64_t* out_len);
int qm_sam_records(const qm_index* ix, int64_t n, const char* names1, const int64_t* name_off1, const char* seq1,
                   const int64_t* off1, const char* names2, const int64_t* name_off2, const char* seq2,
                   const int64_t* off2, const int64_t* hit_offsets, const qm_hit* hits, int32_t max_num_hits,
                   int32_t n_threads, char** out, int64_t* out_len);
/* the same text written straight to an open file descriptor (no copy through the caller); formatted by n_threads
 * workers, written in order by the calling thread */
int qm_sam_write(const qm_index* ix, int64_t n, const char* names1, const int64_t* name_off1, const char* seq1,
                 const int64_t* off1, const char* names2, const int64_t* name_off2, const char* seq2,
                 const int64_t* off2, const int64_t* hit_offsets, const qm_hit* hits, int32_t max_num_hits,
                 int32_t n_threads, int fd, int64_t* bytes_written);
/* A writer for a whole run: qm_sam_writer_put formats a batch with the writer's worker threads and returns; a thread of
 * the writer's own puts the text on the descriptor in batch order while the caller fetches and formats the next batch
 * (two batches of text are buffered; put blocks while both wait).  The batch's arrays are not referenced after put
 * returns.  A write error is reported by the next put and by close; close drains, reports the bytes written and
 * releases the writer (the descriptor stays the caller's). */
typedef struct qm_sam_writer qm_sam_writer;
int qm_sam_writer_open(const qm_index* ix, int fd, int32_t max_num_hits, int32_t n_threads, qm_sam_writer** out);
/* flags: QM_SAM_GZIP = `-x / --compressed` (src/RapMapSAMapper.cpp:832-833 wraps the output buffer in a zstr::ostream, i.e. a
 * zlib deflate stream): every formatter part becomes a gzip member of its own, compressed by the worker that formatted it,
 * written in order -- the concatenation is one valid .gz stream.  Bits 8-11: deflate level 1..9 (0: level 1).
 * qm_sam_writer_header puts the SAM header through the same queue (compressed like everything else). */
#define QM_SAM_GZIP 1u
int qm_sam_writer_open_ex(const qm_index* ix, int fd, int32_t max_num_hits, int32_t n_threads, uint32_t flags, qm_sam_writer** out);
int qm_sam_writer_header(qm_sam_writer* w);
int qm_sam_writer_put(qm_sam_writer* w, int64_t n, const char* names1, const int64_t* name_off1, const char* seq1,
                      const int64_t* off1, const char* names2, const int64_t* name_off2, const char* seq2,
                      const int64_t* off2, const int64_t* hit_offsets, const qm_hit* hits);
int qm_sam_writer_close(qm_sam_writer* w, int64_t* bytes_written);
void qm_buf_free(char* p);

#ifdef __cplusplus
}
#endif
#endif /* QMAP_MI355_H */
