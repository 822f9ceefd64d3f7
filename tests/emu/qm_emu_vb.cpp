// tests/emu/qm_emu_vb.cpp -- TEST-ONLY lane emulation of the variational Bayes method: the two drivers (qm_quant_host.inl,
// qm_boot_host.inl) and the device code of qm_quant.inl and qm_boot.inl compiled with -DQM_EMU, as qm_emu_quant.cpp and
// qm_emu_boot.cpp compile them, in ONE library, so that a quant object, its method and the boot objects that borrow it live
// together.  What is added here is a C face over what the other two do not expose: the method, E over an array, and the
// snapshot's class side of a quant object.
#include "qm_emu_boot.cpp"

extern "C" {

int qe_quant_set_method(void* h, int method, const double* prior) { return quant_set_method((qm_quant*)h, method, prior); }
int qe_exp_digamma(const double* x, long long n, double* out) { return quant_exp_digamma_array(0, x, n, out); }
int qe_quant_classes(void* h, long long* off, u32* tids, uint64_t* cnt) { return quant_fetch_classes((qm_quant*)h, (int64_t*)off, tids, cnt); }

}  // extern "C"
