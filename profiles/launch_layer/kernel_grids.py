"""profiles/launch_layer/kernel_grids.py DIR_A DIR_B -- the kernel traces rocprofv3 wrote under the two directories (launch_all.py with two
libraries) as sorted multisets of (kernel name, grid size, workgroup size), and whether the two are equal.  Launch order is not compared:
the parts of a split call run on streams of their own.  Exit status 1 when they differ."""
import collections
import csv
import glob
import os
import sys


def multiset(d):
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        sys.exit("no *kernel_trace.csv under " + d)
    c = collections.Counter()
    for f in files:
        for r in csv.DictReader(open(f, newline="")):
            pick = lambda *names: next(r[k] for k in names if k in r)
            c[(r["Kernel_Name"], int(pick("Grid_Size_X", "Grid_Size")), int(pick("Workgroup_Size_X", "Workgroup_Size")))] += 1
    return c


def main():
    a, b = multiset(sys.argv[1]), multiset(sys.argv[2])
    print("# kernel | grid size (work-items, x) | workgroup size (x) | dispatches: %s | dispatches: %s" % (sys.argv[1], sys.argv[2]))
    for k in sorted(set(a) | set(b)):
        print("%s | %d | %d | %d | %d%s" % (k[0], k[1], k[2], a[k], b[k], "" if a[k] == b[k] else "   <-- differs"))
    same = a == b
    print("# %d dispatches of %d distinct (kernel, grid, workgroup) against %d of %d: %s" % (
        sum(a.values()), len(a), sum(b.values()), len(b), "IDENTICAL multisets" if same else "DIFFERENT"))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
