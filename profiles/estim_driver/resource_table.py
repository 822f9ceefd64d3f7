"""profiles/estim_driver/resource_table.py -- a build log made with -Rpass-analysis=kernel-resource-usage -> one line per estimation
kernel (the equivalence-class table, the EM, the bootstrap, the fragment-length histogram): SGPRs, VGPRs, scratch, occupancy, spills, LDS.
  make -C rapmap_amd/csrc CXXFLAGS='<the Makefile's> -Rpass-analysis=kernel-resource-usage' 2> build.log
  python profiles/estim_driver/resource_table.py build.log
rocPRIM's kernels and the mapping kernels are left out; a wave body launched through qm_exec.h is named by its body."""
import re
import subprocess
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")
WANT = re.compile(r"(eqc|quant|boot|fld|lib|gcb)_\w+")


def main(path):
    names, rows, cur = [], {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1); names.append(cur); rows[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\S+) \[-Rpass", line)
        if m and cur:
            rows[cur][m.group(1).strip()] = m.group(2)
    plain = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True).stdout.split("\n")
    out = {}
    for mangled, name in zip(names, plain):
        if "rocprim" in name or not WANT.search(name):
            continue
        body = re.search(r"(?:wave2?|sweep)_kernelITnDaXadL_Z(?:NS_)?(\d+)", mangled)          # (the body's name, read from the mangled one)
        if body:
            key = mangled[body.end():body.end() + int(body.group(1))]
            agg = re.match(r"ILi(\d)E", mangled[body.end() + int(body.group(1)):])
            key += "<%s>" % agg.group(1) if agg else ""
            key += "  (wave2_kernel)" if "wave2_kernel" in mangled else "  (sweep_kernel)" if "sweep_kernel" in mangled else "  (wave_kernel)"
        else:
            key = re.sub(r"\(.*", "", name).replace("void ", "")
        out[key] = rows[mangled]
    print("%-40s %5s %5s %7s %4s %6s %6s %6s" % ("kernel", "sgpr", "vgpr", "scratch", "occ", "sspill", "vspill", "lds"))
    for key in sorted(out):
        print("%-40s %5s %5s %7s %4s %6s %6s %6s" % ((key,) + tuple(out[key].get(f, "?") for f in FIELDS)))


if __name__ == "__main__":
    main(sys.argv[1])
