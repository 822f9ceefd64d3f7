// qm_device.h -- the launch layer between qm_host.hip and the kernel units: one typed launcher per kernel family (defined where the
// kernels are, qm_kernels*.hip) and the resident-blocks query their grids start from (the grid arithmetic itself: qm_grid.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <cstdio>
#include <cstdlib>
#include "qm_grid.h"

// waves per SIMD the register allocator must leave room for, per flavour of the stage-A kernel (reads <= 128 bp)
#define QM_SEL_CHUNKS_B 4      // -s: chunks of units the plan -> ksw2 -> finish kernels go through (host side)
#define QMK_DEFAULT_WPS 8
#define QMK_WPS_PH 6
#define QMK_WPS_NIP 8
#define QMK_WPS_PHNIP 6

namespace qm {
struct DevIndex; struct ReadBatch; struct PairBatch; struct SelBatch;   // the launch arguments (qm_mapper.inl, qm_sel.inl)
struct EqcSrc;              // ... of the equivalence-class table (qm_eqc.inl)

// Resident blocks per CU of kernel K launched with THREADS threads: the occupancy query, once per instantiation (FALLBACK where it
// fails); KNOB: QM_BLOCKS_PER_CU -- a tuning knob, fewer resident blocks than the occupancy allows -- may lower it.  See qm_grid.h.
template <auto K, int THREADS, int FALLBACK, bool KNOB>
inline int resident_per_cu() {
  static const int nb = [] {
    int v = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, K, THREADS, 0) != hipSuccess || v < 1) v = FALLBACK;
    const char* ov = KNOB ? getenv("QM_BLOCKS_PER_CU") : nullptr;
    if (ov && atoi(ov) > 0 && atoi(ov) < v) v = atoi(ov);
    return v;
  }();
  return nb;
}
// The same for the two headline kernels, in the unit their grids are counted in -- four waves (qm_grid.h) -- whatever QM_WG_WAVES their
// workgroups have: the query counts workgroups, QM_BLOCKS_PER_CU lowers the units.  QM_GRID_TRACE=1: what the query said, on stderr.
template <auto K, int FALLBACK>
inline int resident_quads_per_cu(const char* name) {
  static const int nq = [name] {
    int v = 0;
    const bool asked = hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, K, 64 * QM_WG_WAVES, 0) == hipSuccess && v >= 1;
    if (getenv("QM_GRID_TRACE")) fprintf(stderr, "[qm grid] %s: %d workgroups of %d wave(s) resident per CU%s\n", name, asked ? v : 0, QM_WG_WAVES, asked ? "" : " (the query failed)");
    v = asked ? v * QM_WG_WAVES / 4 : FALLBACK;
    if (v < 1) v = 1;
    const char* ov = getenv("QM_BLOCKS_PER_CU");
    if (ov && atoi(ov) > 0 && atoi(ov) < v) v = atoi(ov);
    return v;
  }();
  return nq;
}
}  // namespace qm

hipError_t qmk_build_sainfo(const unsigned int* SA, long long nSA, const unsigned int* offsets, long long T, void* out, hipStream_t st);
hipError_t qmk_build_saext(const unsigned char* text, long long n, const unsigned int* SA, long long nSA, int k, const void* sainfo, void* out, hipStream_t st);
hipError_t qmk_build_saext2(const unsigned char* text, long long n, const unsigned int* SA, long long nSA, int k, const void* sainfo, void* out, hipStream_t st);
hipError_t qmk_build_sanext(const unsigned char* text, long long n, const unsigned int* SA, long long nSA, int k, unsigned int* out, hipStream_t st);
hipError_t qmk_build_slots(const void* recs, long long K, void* slots, unsigned long long cap, int k, hipStream_t st);
hipError_t qmk_build_slots_from_ph(const qm::DevIndex& ix, long long n, void* slots, unsigned long long cap, unsigned long long* d_bad, hipStream_t st);
hipError_t qmk_build_phrecs(const unsigned int* data, const unsigned char* lens, long long n, const qm::DevIndex& ix, void* out, hipStream_t st);
hipError_t qmk_build_phfilter(const void* recs, long long n, void* filter, unsigned long long mask, int k, hipStream_t st);
// The launches of the general stage-A kernel (qm_read_kernel.inl), by name.  `ns` is the slot class of the batch (2, 3, 4 or 8 slots of 64
// characters); the stage entry and the two long-read launches have a slot count of their own and ignore it.
enum ReadLaunch {
  RL_FUSED,            // the fused kernel of slot class ns
  RL_CHAIN_COLLECT,    // the chain-scoring collector of slot class ns (first half of a fused -s call)
  RL_ENTRY_COLLECT,    // the collector-only stage entry (qm_collect_reads): eight slots, every read length up to QM_MAX_READ_LEN
  RL_LONG,             // the long-read pass (reads of 513 .. 2048 characters): 32 slots
  RL_LONG_COLLECT      // ... its collector alone
};
hipError_t qmk_map_reads(const qm::DevIndex& ix, const qm::ReadBatch& B, int ns, ReadLaunch what, int grid, int num_cu, hipStream_t st);
// ... the slot classes' units behind it (qm_kernels_ns{2,3,4,8,32}.hip); collect: their collector-only kernels
hipError_t qmk_launch_reads_ns2(const qm::DevIndex& ix, const qm::ReadBatch& B, bool collect, int grid, int num_cu, hipStream_t st);
hipError_t qmk_launch_reads_ns3(const qm::DevIndex& ix, const qm::ReadBatch& B, bool collect, int grid, int num_cu, hipStream_t st);
hipError_t qmk_launch_reads_ns4(const qm::DevIndex& ix, const qm::ReadBatch& B, bool collect, int grid, int num_cu, hipStream_t st);
hipError_t qmk_launch_reads_ns8(const qm::DevIndex& ix, const qm::ReadBatch& B, bool collect, int grid, int num_cu, hipStream_t st);
hipError_t qmk_launch_reads_ns32(const qm::DevIndex& ix, const qm::ReadBatch& B, bool collect, int grid, int num_cu, hipStream_t st);
// the lean stage-A kernel (qm_kernels_lean.hip): reads of up to 128 clean characters, two per wavefront and iteration
hipError_t qmk_launch_lean(const qm::DevIndex& ix, const qm::ReadBatch& B, int num_cu, hipStream_t st);
// ... its N-aware edition over the queue B.slowq[0 .. nreads) (qm_kernels_leanq.hip)
hipError_t qmk_launch_lean_nq(const qm::DevIndex& ix, const qm::ReadBatch& B, int num_cu, hipStream_t st);
// the pair kernel (qm_kernels_duo.hip): the two mates of a pair of up to 128 clean characters each in lockstep in one wavefront, merged there
hipError_t qmk_launch_duo(const qm::DevIndex& ix, const qm::ReadBatch& B, int num_cu, hipStream_t st);
// the one-read-per-wavefront list kernel (hits -> mappings; -s: with chaining) over the collectors' intervals
hipError_t qmk_h2m(const qm::DevIndex& ix, const qm::ReadBatch& B, int grid, int num_cu, hipStream_t st);
// the -s list kernel, several reads per wavefront; reads it leaves for qmk_h2m are queued in todoq (count: scalar slot QM_SC_TODO)
// ... its wide edition over the queue `ids` (*nids entries) the narrow kernel left; what it hands on goes to todoq (count: QM_SC_TODO2)
hipError_t qmk_h2m_packw(const qm::DevIndex& ix, const qm::ReadBatch& B, const long long* ids, const unsigned long long* nids, long long* todoq, int grid, int num_cu, hipStream_t st);
hipError_t qmk_h2m_pack(const qm::DevIndex& ix, const qm::ReadBatch& B, long long* todoq, int grid, int num_cu, hipStream_t st);
hipError_t qmk_sel_merge(const qm::PairBatch& P, const qm::SelBatch& A, hipStream_t st);
// the reads whose lcnt word is `mark` (QM_LCNT_SLOW, QM_LCNT_LEAN) -> q[0 .. min(*count, cap)); the caller zeroes *count first
hipError_t qmk_collect_marked(const unsigned int* lcnt, long long nreads, unsigned int mark, long long* q, long long cap, unsigned long long* count, hipStream_t st);
hipError_t qmk_sel_slots(const qm::PairBatch& P, hipStream_t st);
hipError_t qmk_sel_plan(const qm::PairBatch& P, const qm::SelBatch& A, int num_cu, hipStream_t st);
hipError_t qmk_sel_align_finish(const qm::PairBatch& P, const qm::SelBatch& A, int num_cu, hipStream_t st);
size_t qmk_sel_gmem_rows_bytes(int num_cu);   // device memory of qm_sel_align_gmem_kernel's alignment blocks (long reads under a band beyond 97)
hipError_t qmk_sel_compact(const qm::PairBatch& P, const void* tmp, const void* toff, hipStream_t st);
hipError_t qmk_pair_count(const qm::PairBatch& P, hipStream_t st);
hipError_t qmk_pair_write(const qm::PairBatch& P, hipStream_t st);
// 2-bit packed reads -> the ASCII image the kernels read (include/qmap_mi355.h, "2-bit packed reads"): groups of four, then exceptions
hipError_t qmk_unpack_reads(const unsigned char* packed, const long long* off, long long n, long long total_chars, unsigned char* seq,
                            const void* exc, long long n_exc, hipStream_t st);
size_t qmk_scan_temp_bytes(long long n);
// offs[i] = init + cnt[0] + ... + cnt[i - 1], i < n (init: the hits in front of a part of a split call, map_device_split; otherwise 0)
hipError_t qmk_scan_counts(void* temp, size_t temp_bytes, const unsigned int* cnt, long long* offs, long long n, long long init,
                           hipStream_t st);
// the same over (cnt & 0x7fffffff): list lengths carry the foundHit flag in bit 31
hipError_t qmk_scan_counts_masked(void* temp, size_t temp_bytes, const unsigned int* cnt, long long* offs, long long n, hipStream_t st);
// per read: its interval records and list words from their bump-allocated homes to CSR order (qm_fetch_stages)
hipError_t qmk_stage_gather(long long nreads, const unsigned int* ivcnt, const long long* ivoff, const void* iv, const long long* ivcsr, void* iv_out,
                            const unsigned int* lcnt, const long long* loff, const unsigned long long* lists, const long long* lcsr,
                            unsigned long long* words_out, hipStream_t st);

// The estimation objects' kernels that are neither a plain wave body nor a persistent sweep (those two kinds are launched through
// qm_exec.h where their driver is compiled): the equivalence-class table's.  The lane emulation defines these launchers a second time,
// static, next to the driver (qm_eqc_host.inl).
hipError_t qmk_eqc_label_queued(const qm::EqcSrc& src, long long nq, hipStream_t st);
hipError_t qmk_eqc_reset_probes(unsigned long long* q, long long n, hipStream_t st);
hipError_t qmk_eqc_sum(const unsigned long long* count, const unsigned long long* key, long long cap, unsigned long long* out, hipStream_t st);
