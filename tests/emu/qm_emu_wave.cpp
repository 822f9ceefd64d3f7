// tests/emu/qm_emu_wave.cpp -- TEST-ONLY lane emulation of the primitives by themselves: tests/device/qm_wave_probe.inl (one call of every primitive
// of rapmap_amd/csrc/qm_wave.h, and key_count of qm_selpack.inl) compiled with -DQM_EMU, as a loop over the caller's waves.  The same body is a
// kernel in tests/device/qm_probe.hip; the arguments and the output layout of qe_wave are those of its qp_wave.
#define QM_EMU
#include "../device/qm_wave_probe.inl"

#include <string.h>

using namespace qm;

extern "C" {

int qe_n_ops(void) { return QP_NOPS; }
const char* qe_op_name(int op) {
#define QP_NAME(n) #n,
  static const char* const names[] = {QP_OPS(QP_NAME)};
#undef QP_NAME
  return op >= 0 && op < QP_NOPS ? names[op] : nullptr;
}
int qe_memb(void) { return QP_MEMB; }
int qe_nout(void) { return QP_NOUT; }

// nw waves of op: prm[nw], a / b / c / d [nw * 64], mem[nw * QP_MEMB], atom[nw] (in: the words' start values, out: what the wave left),
// out[nw * QP_NOUT * 64] (filled with the byte 0xEE first).  Returns 0, -1 for a bad argument.
int qe_wave(int op, int nw, const int* prm, const u64* a, const u64* b, const u64* c, const u64* d, const unsigned char* mem, u64* atom, u64* out) {
  if (op < 0 || op >= QP_NOPS || nw < 1) return -1;
  memset(out, 0xEE, (size_t)nw * QP_NOUT * 64 * sizeof(u64));
  for (int w = 0; w < nw; ++w) {
    u32 lds[QP_LDSB / 4];
    memset(lds, 0xCD, sizeof(lds));
    const size_t o = (size_t)w * 64;
    if (probe_wave(op, prm[w], a + o, b + o, c + o, d + o, mem + (size_t)w * QP_MEMB, atom + w, lds, out + o * QP_NOUT)) return -1;
  }
  return 0;
}

}  // extern "C"
