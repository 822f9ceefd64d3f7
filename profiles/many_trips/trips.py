"""profiles/many_trips/results/trips.txt from the log of `pytest -m gpu -s tests/test_many_trips_gpu.py`: per leg and option set the
kernel of the first launch (tests/tile_cases.LEGS), the device's compute units, the widest grid, copies, units and trips per wavefront as
tile_cases worked them out on the device, and what the run reported about the N-aware pass and the kernels of -s.

    python profiles/many_trips/trips.py profiles/many_trips/results/gpu_suite.log > profiles/many_trips/results/trips.txt"""
import os
import re
import sys

sys.path[:0] = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests")]
import conftest  # noqa: F401  (the search path of the test modules)
import tile_cases as tc

LEG = re.compile(r"^\.?(\S+) (\S+): (\d+) CUs, (\d+) wavefronts, (\d+) copies of (\d+) = (\d+) units, (\d+) to (\d+) trips per wavefront(.*?); untiled call and tiling ([\d.]+) s, tiled call and checks ([\d.]+) s")
SMALL = re.compile(r"^\.?(\S+?)\.(\S+): smallest grid(?: -s)?, (\d+) wavefronts, (\d+) copies of (\d+) units, (\d+) to (\d+) trips per wavefront")


def main(path):
    legs = {l.id: l for l in tc.LEGS}
    name = {"pair": "qm_duo_kernel", "lean": "qm_lean_kernel", "general": "qm_read_kernel"}
    label = lambda leg, variant: name[leg.kernel] + (" -s" if variant.startswith(("selAln", "mimic")) else "") + (" wide" if leg.wide else "") + (" compact -p" if leg.compact else "")
    rows, small, notes = [], [], []
    cus = "?"
    for line in open(path):
        m = LEG.match(line)
        if m:
            leg = legs[m.group(1)]
            k = label(leg, m.group(2))
            rows.append((m.group(1), m.group(2), k, m.group(3), m.group(4), m.group(5), m.group(7), "%s-%s" % (m.group(8), m.group(9)), "%.2f" % (float(m.group(11)) + float(m.group(12)))))
            cus = m.group(3)
            if m.group(10):
                notes.append("%s %s%s" % (m.group(1), m.group(2), m.group(10).replace("; ", "\n    ")))
        m = SMALL.match(line)
        if m:
            small.append((m.group(1), m.group(2), label(legs[m.group(1)], m.group(2)), cus, m.group(3), m.group(4), str(int(m.group(4)) * int(m.group(5))), "%s-%s" % (m.group(6), m.group(7)), ""))
    # every leg and option set of tile_cases.LEGS must be in the log: a changed print format must not quietly empty the table
    want = [(l.id, v) for l in tc.LEGS for v in l.variants]
    missing = [x for x in want if x not in [r[:2] for r in rows]] + [("smallest grid",) + x for x in want if legs[x[0]].small and x not in [r[:2] for r in small]]
    if missing:
        sys.exit("trips.py: not in %s: %r" % (path, missing))
    head = ("leg", "option set", "first launch", "CUs", "wavefronts", "copies", "units", "trips/wave", "seconds")
    for title, table in (("widest grid (no knob set)", rows), ("smallest grid (QM_BLOCKS_PER_CU=1 QM_GRID_OVERSUB=1 QM_DUO_OVERSUB=1, a child process)", small)):
        w = [max(len(r[i]) for r in [head] + table) for i in range(len(head))]
        print(title)
        for r in [head] + table:
            print("  " + "  ".join(c.ljust(w[i]) for i, c in enumerate(r)).rstrip())
        print()
    print("reported by the run, no condition but the N-aware pass's six trips:")
    for n in notes:
        print("  " + n)


if __name__ == "__main__":
    main(sys.argv[1])
