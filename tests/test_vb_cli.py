"""quasimap --quant --quantVB [--quantVBPrior P] [--quantPerTranscriptPrior] against Quant under the same prior array, with --quantFLD
and --numBootstraps, and a run without --quantVB against what the EM's own faces write.  Run on the MI355X box: -m gpu."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import quant_cases as qc
import vb_cases as vc
from conftest import GOLD, ROOT
from util import pack

pytestmark = pytest.mark.gpu


def _cli(args):
    r = subprocess.run([sys.executable, "-m", "rapmap_amd", "quasimap"] + args, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r


def _sample_args(sample_data):
    sd = os.path.join(GOLD, "sample_data")
    return ["-i", sample_data["idx"], "-1", os.path.join(sd, "reads_1.fastq.gz"), "-2", os.path.join(sd, "reads_2.fastq.gz"), "-t", "4", "-n"]


def test_cli_quant_vb(sample_data, tmp_path):
    import rapmap_amd as ra
    qf, qp = str(tmp_path / "q.sf"), str(tmp_path / "qp.sf")
    r = _cli(_sample_args(sample_data) + ["--quant", qf, "--quantVB"])
    assert "VBEM iterations, prior 0.01 per nucleotide" in r.stderr
    r = _cli(_sample_args(sample_data) + ["--quant", qp, "--quantVB", "--quantVBPrior", "1e-3", "--quantPerTranscriptPrior"])
    assert "VBEM iterations, prior 0.001 per transcript" in r.stderr
    qi = ra.QuasiIndex(sample_data["idx"])
    mp = ra.QuasiMapper(qi, 0)
    q1, o1 = pack(sample_data["reads1"]); q2, o2 = pack(sample_data["reads2"])
    mp.map_pairs(q1, o1, q2, o2)
    t = ra.EqClasses(mp); t.add(mp)
    lens = np.asarray(qi.txp_lens, dtype=np.float64)
    for path, prior in ((qf, 1e-2 * lens), (qp, np.full(qi.n_txps, 1e-3))):
        q = ra.Quant(t, qi.n_txps, lens)
        q.set_method("vbem", prior=prior)
        q.run()
        names, l2, e2, tpm, reads = ra.read_quant(path)
        assert names == qi.txp_names and np.array_equal(e2, lens)
        vc.assert_close(reads, q.fetch(), "--quantVB against Quant under the same prior array (%s)" % os.path.basename(path))
        assert abs(float(tpm.sum()) - 1e6) <= 1e-6
        q.close()
    t.close(); mp.close()


def test_cli_quant_vb_with_fld(sample_data, tmp_path):
    """the per-nucleotide prior is built from the effective lengths that were learnt, not from the lengths"""
    import rapmap_amd as ra
    qf, ef = str(tmp_path / "q.sf"), str(tmp_path / "eq.txt")
    _cli(_sample_args(sample_data) + ["-q", "--quant", qf, "--quantFLD", "--quantVB", "--eqClasses", ef, "--quantMaxIter", "40", "--quantRelTol", "0"])
    names, lens, eff, tpm, reads = ra.read_quant(qf)
    assert not np.array_equal(eff, lens.astype(np.float64))
    n2, off, tids, cnt = ra.read_eq_classes(ef)
    g = qc.Graph(off, tids, cnt, len(names))
    vc.assert_close(reads, vc.iterate(g, eff, 1e-2 * eff, g.uniform_start(), 40), "--quantFLD --quantVB, 40 iterations")
    by_length = vc.iterate(g, eff, 1e-2 * lens.astype(np.float64), g.uniform_start(), 40)
    assert float(np.abs(reads - by_length).max()) > 1e-6             # (the other prior gives another answer: the comparison above tells them apart)


@pytest.fixture(scope="module")
def small(synth_small, tmp_path_factory):
    """synth_small as FASTQ files, and its table as the device folds it"""
    import rapmap_amd as ra
    d = tmp_path_factory.mktemp("vb_fq")
    f1, f2 = str(d / "r1.fastq"), str(d / "r2.fastq")
    for fn, nms, rds in ((f1, synth_small["names1"], synth_small["reads1"]), (f2, synth_small["names2"], synth_small["reads2"])):
        with open(fn, "wb") as fh:
            for nm, r in zip(nms, rds):
                fh.write(b"@" + nm.encode() + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n")
    qi = ra.QuasiIndex(synth_small["idx"])
    mp = ra.QuasiMapper(qi, 0, debug=False)
    q1, o1 = pack(synth_small["reads1"]); q2, o2 = pack(synth_small["reads2"])
    mp.map_pairs(q1, o1, q2, o2)
    t = ra.EqClasses(mp); t.add(mp)
    g = qc.Graph(*t.fetch(), qi.n_txps)
    t.close()
    yield {"qi": qi, "mp": mp, "g": g, "args": ["-i", synth_small["idx"], "-1", f1, "-2", f2, "-t", "4", "-n", "-q"]}
    mp.close()


@pytest.mark.parametrize("vb", [True, False])
def test_cli_files_against_the_python_faces(small, tmp_path, vb):
    """--quant FILE --numBootstraps 3 with and without --quantVB: quant.sf byte for byte what write_quant writes from Quant, the replicates
    what Quant.bootstrap gives, on a table filled the way the CLI fills its own (a table of the default size, the stream's sorted
    classes in one add_labels: equal input gives equal slots, hence the same snapshot order).  Without --quantVB the expected files
    are made by the EM's faces alone, as before the variational method existed."""
    import rapmap_amd as ra
    qi, g = small["qi"], small["g"]
    nt = qi.n_txps
    qf, mine = str(tmp_path / "q.sf"), str(tmp_path / "mine.sf")
    r = _cli(small["args"] + ["--quant", qf, "--numBootstraps", "3", "--bootstrapSeed", "7"] + (["--quantVB"] if vb else []))
    names, lens, eff, tpm, reads = ra.read_quant(qf)
    t = ra.EqClasses(small["mp"])
    t.add_labels(g.off, g.tid, g.cnt)
    q = ra.Quant(t, nt, eff)
    if vb:
        q.set_method("vbem", prior=1e-2 * eff)
    q.run()
    ra.write_quant(mine, qi.txp_names, lens, eff, q.fetch())
    assert open(qf, "rb").read() == open(mine, "rb").read()
    want = q.bootstrap(3, seed=7)
    assert gzip.open(qf + ".bootstraps.gz", "rb").read() == np.ascontiguousarray(want, dtype="<f8").tobytes()
    assert len(set(x.tobytes() for x in want)) == 3
    q.close(); t.close()
    if not vb:
        assert "VBEM" not in r.stderr
