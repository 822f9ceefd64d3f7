"""profiles/est_objects/api_calls.py -- HIP API calls per fold of qm_fld_add and per sweep of qm_lib_add and qm_gcb_add.
  run TREE fld|lib|gcb N   one small mapped batch, then N calls, with rapmap_amd imported from TREE: the run a HIP trace wraps
                        (rocprofv3 --hip-trace --stats -d DIR/<what>_<N>_<parent|branch> -o t --output-format csv -- python ... run ...)
  table DIR             the table from those runs' t_hip_api_stats.csv at N = 1 and N = 11, parent and branch
profiles/est_objects/run.sh does both."""
import csv
import os
import sys
import tempfile


def run(root, what, n):
    sys.path.insert(0, root)
    import rapmap_amd as ra
    from rapmap_amd import synth
    names, txps = synth.make_transcriptome(60, seed=3)
    s1, s2, off, _ = synth.make_reads(txps, 4000, seed=4)
    with tempfile.TemporaryDirectory() as td:
        fa = os.path.join(td, "t.fa"); synth.write_fasta(fa, names, txps)
        idx = os.path.join(td, "idx"); ra.build_index(fa, idx, threads=4)
        qi = ra.QuasiIndex(idx); mp = ra.QuasiMapper(qi, 0)
        mp.map_pairs(s1, off, s2, off)
        obj = ra.FragLenDist(mp) if what == "fld" else ra.GCBias(mp) if what == "gcb" else ra.LibFormat(mp, "IU")
        for _ in range(n):
            obj.add(mp)
        print(what, n, obj.stat())
        obj.close(); mp.close(); qi.close()


def table(d):
    def load(p):
        return {r["Name"]: int(r["Calls"]) for r in csv.DictReader(open(os.path.join(d, p, "t_hip_api_stats.csv")))}
    print("# rocprofv3 --hip-trace --stats (no counters), runs of their own: one small mapped batch, then N = 1 and N = 11 calls of qm_fld_add")
    print("# (FragLenDist.add), qm_lib_add (LibFormat(\"IU\").add) or qm_gcb_add (GCBias.add).  Per call = (calls at N = 11 - calls at N = 1) / 10; APIs that do not grow with N are left out.")
    for what, name in (("fld", "qm_fld_add, per fold"), ("lib", "qm_lib_add, per sweep"), ("gcb", "qm_gcb_add, per sweep")):
        if not os.path.isdir(os.path.join(d, "%s_1_parent" % what)):
            continue
        print("## %-31s %8s %8s" % (name, "parent", "branch"))
        per = {}
        for t in ("parent", "branch"):
            a = load("%s_1_%s" % (what, t)); b = load("%s_11_%s" % (what, t))
            for k in set(a) | set(b):
                if b.get(k, 0) != a.get(k, 0):
                    per.setdefault(k, {})[t] = (b.get(k, 0) - a.get(k, 0)) / 10
        for k in sorted(per):
            print("%-34s %8g %8g" % (k, per[k].get("parent", 0), per[k].get("branch", 0)))
        p = load("%s_11_parent" % what); b = load("%s_11_branch" % what)
        diff = {k: (p.get(k, 0), b.get(k, 0)) for k in set(p) | set(b) if p.get(k, 0) != b.get(k, 0)}
        print("# whole run at N = 11, APIs whose counts differ between parent and branch: %s" % (diff or "none"))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    else:
        table(sys.argv[2])
