// tests/device/qm_wave_probe.inl -- TEST-ONLY: one wave body that calls every primitive of rapmap_amd/csrc/qm_wave.h (and key_count of
// qm_selpack.inl, and the pieces of the sweep frame of qm_sweep.h) once, written against LV / QM_LANES like every wave body of the product.  It is compiled twice: with -DQM_EMU by
// tests/emu/qm_emu_wave.cpp (a loop over waves on the CPU) and as a kernel by tests/device/qm_probe.hip (one wavefront per wave, four
// wavefronts per block, all 64 lanes active), so the two editions of a primitive see the same input and can be compared bit for bit.
//
// A wave's input: four u64 per lane (a, b, c, d), one wave-uniform int (prm), QP_MEMB bytes of read-only memory (mem, 16-byte aligned),
// one u64 for the atomics (atom), QP_LDSB bytes of LDS (lds).  Its output: QP_NOUT u64 per lane, out[k * 64 + lane]; what an op does not
// write stays as the caller filled it.  Every address into mem is reduced modulo the room here, whatever the caller passes.
#pragma once
#include "../../rapmap_amd/csrc/qm_mapper.inl"
#include "../../rapmap_amd/csrc/qm_lib.inl"     // (qm_sweep.h, and the word maps of the library-type sweep's counter flush)

#define QP_MEMB 4096               // bytes of read-only memory per wave
#define QP_LDSB 4096               // bytes of LDS per wave (slab_flush: the 1024 words of the largest slab)
#define QP_NOUT 16                 // u64 per lane of output (slab_flush: 1024 bins)

#define QP_OPS(X) \
  X(ballot) X(half_ballot) \
  X(read_lane_i32) X(read_lane_u32) X(read_lane_u64) X(read_lane_f64) X(read_lane_w2) X(read_lane_w4) \
  X(uniform_i32) X(uniform_u32) X(uniform_u64) X(uniform_i64) X(uniform_bool) \
  X(wave_max) X(lane_scan_add) X(lane_scan_max) X(lane_rotate_up) X(row_rotate_up) X(row_last) X(row16_shl1) \
  X(row16_scan_max_excl) X(row16_max_all) X(group_min) \
  X(lane_xor1) X(swap32_u32) X(swap32_u64) X(swap32_w2) X(swap32_w4) X(half_read) X(wave_read) X(row8_or) X(half_max) \
  X(group_sum_f64) X(wave_sum_f64) X(quarters_sum_f64) \
  X(ctz64) X(clz64) X(popc64) X(brev64) X(brev32) X(mulhi64) X(lanemask_lt) X(perm8) X(align_bytes) \
  X(pk_add) X(pk_sub) X(pk_max_i) X(pk_max_u) X(pk_min_u) X(load_u32_unaligned) X(load_u64_unaligned) \
  X(load_16) X(load_32) X(load_16x2) X(load_8_16) X(load_48) X(load_uniform_i64) X(lds_dma_u32) X(lds_dma_u128) \
  X(atomic_min_u64) X(atomic_max_u64) X(atomic_or_u64) X(atomic_add_u64) \
  X(key_count) \
  X(unit_bounds) X(flush_counters_1) X(flush_counters_7) X(flush_counters_16) X(flush_counters_lib) X(slab_flush)

namespace qm {

#define QP_ENUM(n) QP_##n,
enum { QP_OPS(QP_ENUM) QP_NOPS };
#undef QP_ENUM

QM_DEV double qp_f64(u64 b) { double x; __builtin_memcpy(&x, &b, 8); return x; }
QM_DEV u64 qp_bits(double x) { u64 b; __builtin_memcpy(&b, &x, 8); return b; }
QM_DEV u64 qp_pair(u32 lo, u32 hi) { return ((u64)hi << 32) | lo; }

// LV<T> x with x[l] = expr, and out[k][l] = expr (l: the lane)
#define QP_LV(T, x, expr) LV<T> x; QM_LANES(l) { x[l] = (T)(expr); }
#define QP_OUT(k, expr) QM_LANES(l) { out[(k) * 64 + l] = (u64)(expr); }
#define QP_OUT_U4(k, v) QM_LANES(l) { out[(k) * 64 + l] = qp_pair(v[l].x, v[l].y); out[((k) + 1) * 64 + l] = qp_pair(v[l].z, v[l].w); }

// flush_counters onto the output's first row as the counter words: accumulator i = a[i] (wave-uniform)
template <int N>
QM_DEV void probe_flush(const u64* a, u64* out, const int (&word)[N]) {
  u64 acc[N];
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = uniform(a[i]);
  flush_counters(out, acc, word);
}
// the arguments unit_bounds is probed with: n = prm units whose n + 1 offsets fit mem, wavefront a[0] of b[0]
#define QP_UNIT_BOUNDS_OK(prm, wave, nWaves) ((prm) >= 1 && (prm) <= QP_MEMB / 8 - 1 && (u64)(nWaves) >= 1 && (u64)(nWaves) <= 64 && (u64)(wave) < (u64)(nWaves))

// returns 0, or -1 for an op it does not know (nothing is written then)
QM_DEV int probe_wave(int op, int prm, const u64* a, const u64* b, const u64* c, const u64* d, const unsigned char* mem, u64* atom, u32* lds,
                      u64* out) {
  switch (op) {
    case QP_ballot: { QP_LV(bool, p, a[l] & 1) const u64 m = ballot(p); QP_OUT(0, m) } break;
    case QP_half_ballot: { QP_LV(bool, p, a[l] & 1) LV<u32> r; half_ballot(p, r); QP_OUT(0, r[l]) } break;
    case QP_read_lane_i32: { QP_LV(int, x, a[l]) const int r = read_lane(x, prm & 63); QP_OUT(0, (u32)r) } break;
    case QP_read_lane_u32: { QP_LV(u32, x, a[l]) const u32 r = read_lane(x, prm & 63); QP_OUT(0, r) } break;
    case QP_read_lane_u64: { QP_LV(u64, x, a[l]) const u64 r = read_lane(x, prm & 63); QP_OUT(0, r) } break;
    case QP_read_lane_f64: { QP_LV(double, x, qp_f64(a[l])) const double r = read_lane(x, prm & 63); QP_OUT(0, qp_bits(r)) } break;
    case QP_read_lane_w2: {
      LV<Wide<2>> x; QM_LANES(l) { x[l].w[0] = a[l]; x[l].w[1] = b[l]; }
      const Wide<2> r = read_lane(x, prm & 63);
      QP_OUT(0, r.w[0]) QP_OUT(1, r.w[1])
    } break;
    case QP_read_lane_w4: {
      LV<Wide<4>> x; QM_LANES(l) { x[l].w[0] = a[l]; x[l].w[1] = b[l]; x[l].w[2] = c[l]; x[l].w[3] = d[l]; }
      const Wide<4> r = read_lane(x, prm & 63);
      QP_OUT(0, r.w[0]) QP_OUT(1, r.w[1]) QP_OUT(2, r.w[2]) QP_OUT(3, r.w[3])
    } break;
    // uniform(): the caller passes one value in all 64 lanes (the precondition)
    case QP_uniform_i32: { QP_OUT(0, (u32)uniform((int)a[l])) } break;
    case QP_uniform_u32: { QP_OUT(0, uniform((u32)a[l])) } break;
    case QP_uniform_u64: { QP_OUT(0, uniform((u64)a[l])) } break;
    case QP_uniform_i64: { QP_OUT(0, uniform((long long)a[l])) } break;
    case QP_uniform_bool: { QP_OUT(0, uniform((bool)(a[l] & 1)) ? 1 : 0) } break;
    case QP_wave_max: { QP_LV(int, x, a[l]) const int m = wave_max(x); QP_OUT(0, (u32)m) } break;
    case QP_lane_scan_add: { QP_LV(int, x, a[l]) lane_scan_add(x); QP_OUT(0, (u32)x[l]) } break;
    case QP_lane_scan_max: { QP_LV(int, x, a[l] & 0x7fffffffu) lane_scan_max(x); QP_OUT(0, (u32)x[l]) } break;   // (values >= 0)
    case QP_lane_rotate_up: { QP_LV(int, x, a[l]) LV<int> r; lane_rotate_up(x, r); QP_OUT(0, (u32)r[l]) } break;
    case QP_row_rotate_up: { QP_LV(int, x, a[l]) LV<int> r; row_rotate_up(x, r); QP_OUT(0, (u32)r[l]) } break;
    case QP_row_last: { QP_LV(int, x, a[l]) LV<int> r; row_last(x, r); QP_OUT(0, (u32)r[l]) } break;
    case QP_row16_shl1: { QP_LV(int, x, a[l]) LV<int> r; row16_shl1(x, r, prm); QP_OUT(0, (u32)r[l]) } break;
    case QP_row16_scan_max_excl: { QP_LV(int, x, a[l]) row16_scan_max_excl(x, prm); QP_OUT(0, (u32)x[l]) } break;
    case QP_row16_max_all: { QP_LV(int, x, a[l]) row16_max_all(x); QP_OUT(0, (u32)x[l]) } break;
    case QP_group_min: {
      const int G = prm;
      if (G != 1 && G != 2 && G != 4 && G != 8 && G != 16 && G != 32 && G != 64) return -1;
      QP_LV(int, x, a[l]) group_min(x, G); QP_OUT(0, (u32)x[l])
    } break;
    case QP_lane_xor1: { QP_LV(u32, x, a[l]) LV<u32> r; lane_xor1(x, r); QP_OUT(0, r[l]) } break;
    case QP_swap32_u32: { QP_LV(u32, x, a[l]) LV<u32> r; swap32(x, r); QP_OUT(0, r[l]) } break;
    case QP_swap32_u64: { QP_LV(u64, x, a[l]) LV<u64> r; swap32(x, r); QP_OUT(0, r[l]) } break;
    case QP_swap32_w2: {
      LV<Wide<2>> x, r; QM_LANES(l) { x[l].w[0] = a[l]; x[l].w[1] = b[l]; }
      swap32(x, r);
      QP_OUT(0, r[l].w[0]) QP_OUT(1, r[l].w[1])
    } break;
    case QP_swap32_w4: {
      LV<Wide<4>> x, r; QM_LANES(l) { x[l].w[0] = a[l]; x[l].w[1] = b[l]; x[l].w[2] = c[l]; x[l].w[3] = d[l]; }
      swap32(x, r);
      QP_OUT(0, r[l].w[0]) QP_OUT(1, r[l].w[1]) QP_OUT(2, r[l].w[2]) QP_OUT(3, r[l].w[3])
    } break;
    case QP_half_read: { QP_LV(u32, x, a[l]) QP_LV(int, i, b[l]) LV<u32> r; half_read(x, i, r); QP_OUT(0, r[l]) } break;
    case QP_wave_read: { QP_LV(u32, x, a[l]) QP_LV(int, i, b[l]) LV<u32> r; wave_read(x, i, r); QP_OUT(0, r[l]) } break;
    case QP_row8_or: { QP_LV(u32, x, a[l]) row8_or(x); QP_OUT(0, x[l]) } break;
    case QP_half_max: { QP_LV(int, x, a[l]) half_max(x); QP_OUT(0, (u32)x[l]) } break;
    case QP_group_sum_f64: {
      if (prm != 8 && prm != 16) return -1;
      QP_LV(double, x, qp_f64(a[l])) group_sum_f64(x, prm); QP_OUT(0, qp_bits(x[l]))
    } break;
    case QP_wave_sum_f64: { QP_LV(double, x, qp_f64(a[l])) const double s = wave_sum_f64(x); QP_OUT(0, qp_bits(s)) } break;
    case QP_quarters_sum_f64: { QP_LV(double, x, qp_f64(a[l])) quarters_sum_f64(x); QP_OUT(0, qp_bits(x[l])) } break;
    case QP_ctz64: { QP_OUT(0, (u32)ctz64(a[l])) } break;
    case QP_clz64: { QP_OUT(0, (u32)clz64(a[l])) } break;
    case QP_popc64: { QP_OUT(0, (u32)popc64(a[l])) } break;
    case QP_brev64: { QP_OUT(0, brev64(a[l])) } break;
    case QP_brev32: { QP_OUT(0, brev32((u32)a[l])) } break;
    case QP_mulhi64: { QP_OUT(0, mulhi64(a[l], b[l])) } break;
    case QP_lanemask_lt: { QP_OUT(0, lanemask_lt((int)(a[l] & 63))) } break;
    case QP_perm8: { QP_OUT(0, perm8((u32)a[l], (u32)b[l], (u32)c[l])) } break;
    case QP_align_bytes: { QP_OUT(0, align_bytes((u32)a[l], (u32)b[l], (int)(c[l] & 3))) } break;
    case QP_pk_add: { QP_OUT(0, pk_add((u32)a[l], (u32)b[l])) } break;
    case QP_pk_sub: { QP_OUT(0, pk_sub((u32)a[l], (u32)b[l])) } break;
    case QP_pk_max_i: { QP_OUT(0, pk_max_i((u32)a[l], (u32)b[l])) } break;
    case QP_pk_max_u: { QP_OUT(0, pk_max_u((u32)a[l], (u32)b[l])) } break;
    case QP_pk_min_u: { QP_OUT(0, pk_min_u((u32)a[l], (u32)b[l])) } break;
    case QP_load_u32_unaligned: { QP_OUT(0, load_u32_unaligned(mem + a[l] % (QP_MEMB - 8))) } break;
    case QP_load_u64_unaligned: { QP_OUT(0, load_u64_unaligned(mem + a[l] % (QP_MEMB - 8))) } break;
    case QP_load_16: { LV<U4> v; QM_LANES(l) { v[l] = load_16(mem + 16 * (a[l] % (QP_MEMB / 16))); } QP_OUT_U4(0, v) } break;
    case QP_load_32: {
      LV<U4> v, w; QM_LANES(l) { load_32(mem + 16 * (a[l] % (QP_MEMB / 16 - 1)), v[l], w[l]); }
      QP_OUT_U4(0, v) QP_OUT_U4(2, w)
    } break;
    case QP_load_16x2: {
      LV<U4> v, w; QM_LANES(l) { load_16x2(mem + 16 * (a[l] % (QP_MEMB / 16)), mem + 16 * (b[l] % (QP_MEMB / 16)), v[l], w[l]); }
      QP_OUT_U4(0, v) QP_OUT_U4(2, w)
    } break;
    case QP_load_8_16: {
      LV<u64> v; LV<U4> w;
      QM_LANES(l) { load_8_16((const u64*)mem + a[l] % (QP_MEMB / 8), (const u64*)(mem + 16 * (b[l] % (QP_MEMB / 16))), v[l], w[l]); }
      QP_OUT(0, v[l]) QP_OUT_U4(1, w)
    } break;
    case QP_load_48: {
      LV<U4> v, w, x; QM_LANES(l) { load_48(mem + 16 * (a[l] % (QP_MEMB / 16 - 2)), v[l], w[l], x[l]); }
      QP_OUT_U4(0, v) QP_OUT_U4(2, w) QP_OUT_U4(4, x)
    } break;
    case QP_load_uniform_i64: { const long long v = load_uniform_i64((const long long*)mem + (u32)prm % (QP_MEMB / 8)); QP_OUT(0, v) } break;
    // a scattered global address per lane, one LDS base for the wave, the LDS read back after the wait
    case QP_lds_dma_u32: {
      QM_LANES(l) { lds_dma_u32((const u32*)mem + a[l] % (QP_MEMB / 4), lds, l); }
      lds_dma_wait();
      QP_OUT(0, lds[l])
    } break;
    case QP_lds_dma_u128: {
      QM_LANES(l) { lds_dma_u128(mem + 16 * (a[l] % (QP_MEMB / 16)), lds, l); }
      lds_dma_wait();
      QP_OUT(0, qp_pair(lds[4 * l], lds[4 * l + 1])) QP_OUT(1, qp_pair(lds[4 * l + 2], lds[4 * l + 3]))
    } break;
    // all 64 lanes on the wave's one word; the caller looks at the word afterwards (the order of the lanes is not defined)
    case QP_atomic_min_u64: { QM_LANES(l) { atomic_min_u64(atom, a[l]); } } break;
    case QP_atomic_max_u64: { QM_LANES(l) { atomic_max_u64(atom, a[l]); } } break;
    case QP_atomic_or_u64: { QM_LANES(l) { atomic_or_u64(atom, a[l]); } } break;
    case QP_atomic_add_u64: { QM_LANES(l) { (void)atomic_add_u64(atom, a[l]); } } break;
    case QP_key_count: { QP_LV(int, n, prm) QM_LANES(l) { key_count(a[l], b[l], c[l], d[l], n[l]); } QP_OUT(0, (u32)n[l]) } break;
    // ---- the sweep frame (qm_sweep.h)
    // mem: the n + 1 offsets as 64-bit values, n = prm; this wave is wavefront a[0] of b[0] and strides as a sweep does: trip k's bounds
    // (off[u], off[u + 1]) go to rows 2 k and 2 k + 1, and a lane past n writes nothing
    case QP_unit_bounds: {
      const long long wave = (long long)uniform(a[0]), nWaves = (long long)uniform(b[0]);
      if (!QP_UNIT_BOUNDS_OK(prm, wave, nWaves)) return -1;
      const UnitSrc S{nullptr, 0, (const long long*)mem, prm, 0};
      int k = 0;
      for (long long base = wave * 64; base < S.n && k < QP_NOUT / 2; base += nWaves * 64, ++k) {
        LV<long long> o0, o1;
        unit_bounds(S, base, o0, o1);
        QM_LANES(l) { if (base + l < S.n) { out[(2 * k) * 64 + l] = (u64)o0[l]; out[(2 * k + 1) * 64 + l] = (u64)o1[l]; } }
      }
    } break;
    // 1, 7 and 16 accumulators and the classify sweep's 15 onto the pre-filled words of row 0
    case QP_flush_counters_1: { const int word[1] = {3}; probe_flush(a, out, word); } break;
    case QP_flush_counters_7: { const int word[7] = {0, 1, 2, 3, 4, 5, 6}; probe_flush(a, out, word); } break;
    case QP_flush_counters_16: { const int word[16] = LIB_UNITS_WORDS; probe_flush(a, out, word); } break;
    case QP_flush_counters_lib: { const int word[15] = LIB_CLASSIFY_WORDS; probe_flush(a, out, word); } break;
    // a slab of QP_LDSB / 4 words: word i < prm holds (u32)(a[i % 64] >> (i / 64)), the others 0xA5A5A5A5; its first prm words go
    // out onto the output taken as QP_NOUT * 64 bins
    case QP_slab_flush: {
      if (prm < 1 || prm > QP_LDSB / 4) return -1;
      QM_LDS(u32)* slab = (QM_LDS(u32)*)lds;
      QM_LANES(l) { for (int i = l; i < QP_LDSB / 4; i += 64) slab[i] = i < prm ? (u32)(a[l] >> (i >> 6)) : 0xA5A5A5A5u; }
      slab_flush(slab, prm, out);
    } break;
    default: return -1;
  }
  return 0;
}

#undef QP_LV
#undef QP_OUT
#undef QP_OUT_U4

}  // namespace qm
