"""Indices, reads and checks of the k-mer length tests (test_kmer_lengths.py: the lane emulation of the device source,
test_kmer_lengths_gpu.py: the HIP path): everything that maps a read elsewhere in the suite does so at k = 31.

The reference throughout is the oracle (oracle.Oracle(q5.load(idx))), which reads k from the index header.  The reference's
own quasimap binary cannot be built in this project's image, so there is no golden SAM at another k; truth_check() below is
the one check that does not go through the oracle.

No test functions here.  Indices and read sets are built once per process and kept (mapping_harness.once); the test modules
reach them through module-scoped fixtures that pass a directory of tmp_path_factory's."""
import gzip
import os
import shutil

import numpy as np

import mapping_harness as mh
from conftest import GOLD
from util import pack

KS = (15, 17, 21, 29)              # 15 / 17: either side of the 32 bits of a packed k-mer; 29: next to the maximum; 21: the common choice
K_SMALL = 9                        # nearly every read trips the take-or-leave rule of the pair / lean kernels: default options only, never -s

# Reads the pair kernel and the lean kernel leave to the general kernel on synth_small's golden reads (8 468 of them) under default
# options, per (k, image).  From the lane emulation (QM_EMU_LEAN_STATS), never from the device: test_kmer_lengths.py holds the
# emulation of both kernels to this table, test_kmer_lengths_gpu.py holds qm_ctx_stat(QM_STAT_LEAN_DEFERRED) of both to it.
# ("lean": by its first pass, which is what a call reports when the N-aware pass does not run.  At k = 15 and 17 the pair kernel
# leaves one read more than the lean kernel; at k = 31 both leave 519, the figure test_gpu_parity.py pins.  "ph" is the compact image
# of a -p index on the device -- where the host only ever launches the lean kernel, so its "pair" entry is held by the emulation alone.)
EXPECT_LEFT = {
    (9, "dense"): {"pair": 7901, "lean": 7901},
    (15, "dense"): {"pair": 661, "lean": 660}, (15, "ph"): {"pair": 661, "lean": 660},
    (17, "dense"): {"pair": 626, "lean": 625}, (17, "ph"): {"pair": 626, "lean": 625},
    (21, "dense"): {"pair": 553, "lean": 553}, (21, "ph"): {"pair": 553, "lean": 553},
    (29, "dense"): {"pair": 529, "lean": 529}, (29, "ph"): {"pair": 529, "lean": 529},
}

# the option sets of the golden reads at k = 15, 17 and 29 (at k = 21: every one of mapping_harness.PLAIN_SETS), and the few of the other reads
SOME = ("default", "noStrictCheck", "z0.9", "noSensitive", "fuzzy", "selAln")
FEW = ("default", "noSensitive", "fuzzy", "selAln")


# ---- synth_small (the golden transcriptome and its 4 234 adversarial pairs)

def golden_fasta(tmp_root):
    def make():
        fa = os.path.join(mh.subdir(tmp_root, "golden"), "txome.fa")
        with gzip.open(os.path.join(GOLD, "synth_small", "txome.fa.gz"), "rb") as g, open(fa, "wb") as o:
            shutil.copyfileobj(g, o)
        return fa
    return mh.once("golden_fasta", make)


def index_for(tmp_root, k, image):
    """the synth_small transcriptome indexed at k; image: "dense" or "ph" (`quasiindex -p`)"""
    return mh.once(("golden", k, image), lambda: mh.build(golden_fasta(tmp_root), os.path.join(mh.subdir(tmp_root, "golden"), "idx_k%d_%s" % (k, image)), k, image))


def golden_reads():
    """(names1, reads1, names2, reads2, packed): packed = (q1, o1, q2, o2)"""
    def make():
        import samfmt as sam
        n1, s1 = sam.read_fastq(os.path.join(GOLD, "synth_small", "reads_1.fastq.gz"))
        n2, s2 = sam.read_fastq(os.path.join(GOLD, "synth_small", "reads_2.fastq.gz"))
        return n1, s1, n2, s2, pack(s1) + pack(s2)
    return mh.once("golden_reads", make)


# ---- a smaller transcriptome for reads beyond 128 characters and for the error-free pairs

def small_txome(tmp_root):
    """{"fasta", "names", "txps"}: 60 genes (a few hundred transcripts, about 0.6 M characters), 5 % of them again as paralogs"""
    def make():
        from rapmap_amd import synth
        names, txps = synth.make_transcriptome(60, seed=2121, paralog_frac=0.05)
        fa = os.path.join(mh.subdir(tmp_root, "small"), "txome.fa")
        synth.write_fasta(fa, names, txps)
        assert 100 < len(txps) < 1000 and sum(t.size for t in txps) < 1000000
        return {"fasta": fa, "names": names, "txps": txps}
    return mh.once("small_txome", make)


def small_index(tmp_root, k, image):
    return mh.once(("small", k, image), lambda: mh.build(small_txome(tmp_root)["fasta"], os.path.join(mh.subdir(tmp_root, "small"), "idx_k%d_%s" % (k, image)), k, image))


def long_reads(tmp_root, read_len, n, seed):
    """(q1, o, q2, o) of n pairs of read_len characters off small_txome, 1 % substitutions"""
    def make():
        from rapmap_amd import synth
        txps = [t for t in small_txome(tmp_root)["txps"] if t.size >= 3 * read_len]
        s1, s2, off, _ = synth.make_reads(txps, n, seed=seed, read_len=read_len, err=0.01)
        return s1, off, s2, off
    return mh.once(("long_reads", read_len, n, seed), make)


def index_text(idx):
    """(text uint8[n], transcript starts int64[T]) of an index on disk"""
    import rapmap_amd as ra
    qi = ra.QuasiIndex(idx)
    text, offsets = qi.arrays()
    qi.close()
    return np.asarray(text), np.asarray(offsets, dtype=np.int64)


# ---- reads on the edges that move with k

def edge_lengths(k):
    return [0, 5, k - 1, k, k + 1, k + 2, 2 * k - 1, 2 * k, 2 * k + 1, 63, 64, 65, 99, 100, 101, 126, 127, 128]


EDGE_KINDS = ("plain", "one_N", "run", "two_subst", "lower", "dollar", "swapped", "N_at_k", "N_at_k-1", "N_at_L-k-1", "N_at_k_and_run")


def edge_reads(idx, k, seed=5):
    """test_gpu_parity._lean_edge_reads restated relative to k: mates of every length in edge_lengths(k) (below k, around k and 2 k, around
    the 64- and 128-character slots), each as: a clean fragment, with one N somewhere, with a run of k + 2 equal bases, with two
    substitutions, in lower case, with a `$`, with the mates swapped -- and with an N exactly behind the first k-mer (read position k: the
    first-hit scan passes over that k-mer as well), on the first k-mer's last base (k - 1), at L - k - 1 (the last k-mer's neighbour), and
    at k with k + 2 equal bases right behind it (a window of k equal bases in a read that is not clean; the base varies from read to read).
    Every length meets every kind, once with mates of equal length and once with mate 2 seven lengths further on."""
    def make():
        rng = np.random.default_rng(seed * 1000 + k)
        text, offsets = index_text(idx)
        ends = np.append(offsets[1:], text.size) - 1            # every transcript is followed by `$`
        ok = np.nonzero(ends - offsets >= 300)[0]
        lens = edge_lengths(k)
        r1, r2 = [], []
        for i in range(2 * len(lens) * len(EDGE_KINDS)):
            j, block = i % len(lens), i // len(lens)
            kind = EDGE_KINDS[block % len(EDGE_KINDS)]
            L1 = lens[j]
            L2 = lens[(j + 7) % len(lens)] if block >= len(EDGE_KINDS) else L1
            t = ok[rng.integers(0, ok.size)]
            a = int(offsets[t] + rng.integers(0, ends[t] - offsets[t] - 280))
            f = text[a:a + L1].copy()
            m = mh.COMP[text[a + 150:a + 150 + L2][::-1]].copy()
            for r in (f, m):
                L = r.size
                if L == 0:
                    continue
                if kind == "one_N":
                    r[rng.integers(0, L)] = ord("N")
                if kind == "run" and L > 10:
                    r[10:10 + k + 2] = b"ACGT"[i % 4]
                if kind == "N_at_k_and_run":                    # a dirty read with a window of k equal bases behind its N (any base: an all-A k-mer is the word 0)
                    r[k + 1:2 * k + 3] = b"ACGT"[i % 4]
                if kind == "two_subst":
                    for _ in range(2):
                        r[rng.integers(0, L)] = b"ACGT"[rng.integers(0, 4)]
                if kind == "lower":
                    r[:] = np.frombuffer(bytes(r).lower(), dtype=np.uint8)
                if kind == "dollar" and L > 3:
                    r[rng.integers(0, L)] = ord("$")
                if kind in ("N_at_k", "N_at_k_and_run") and L > k:
                    r[k] = ord("N")
                if kind == "N_at_k-1" and L >= k:
                    r[k - 1] = ord("N")
                if kind == "N_at_L-k-1" and L >= k + 1:
                    r[L - k - 1] = ord("N")
            if kind == "swapped":
                f, m = m, f
            r1.append(bytes(f)); r2.append(bytes(m))
        return r1, r2
    return mh.once(("edge_reads", idx, k, seed), make)


def n_case_reads(idx, k, seed=5):
    """edge_reads' pairs that carry an N"""
    r1, r2 = edge_reads(idx, k, seed)
    keep = [i for i in range(len(r1)) if b"N" in r1[i] or b"N" in r2[i]]
    return [r1[i] for i in keep], [r2[i] for i in keep]


def has_window(read, k):
    """a window of k equal bases (isHomoPolymer's question, asked of the whole read)"""
    r = np.frombuffer(bytes(read).upper(), dtype=np.uint8)
    if r.size < k:
        return False
    run = best = 1
    for i in range(1, r.size):
        run = run + 1 if r[i] == r[i - 1] else 1
        best = max(best, run)
    return best >= k


def run_reads(tmp_root, k):
    """conftest's runs_data restated relative to k.  -> {"fasta", "idx" (dense, at k), "reads1", "reads2"}: transcripts that hold a
    homopolymer run of every length in k - 7 .. k + 9 (and 2 k + 2, 3 k) or a dinucleotide repeat; reads of 100 characters that start
    0 .. 7, 17 and 30 bases before the run, so the run meets every alignment of the four-characters-per-lane packing.  The pair and lean
    kernels leave a read when 4 * (lanes of four equal characters) + 6 >= k, a rule that is necessary for a window of k equal bases and
    not sufficient: runs of k .. k + 9 truly hold such a window, runs of k - 7 .. k - 1 trip the rule at some alignments without one.
    Six starts of every run also carry an N, at the read's first base or right in front of the run, where the walk then starts again on a
    k-mer of k equal bases that the index holds (the homopolymer test of reads that are not clean); the bases of the runs cycle
    through A C G T (an all-A k-mer is the word 0, the others are not).  Also the read of nothing but A, and k A's followed by transcript."""
    def make():
        from rapmap_amd import synth
        rng = np.random.default_rng(4242 + k)
        names, txps, spots = [], [], []
        runs = [(r, False) for r in range(k - 7, k + 10)] + [(2 * k + 2, False), (3 * k, False), (k, True), (k + 1, True), (2 * k, True), (k - 1, False), (k, False)]
        for i, (run, dinuc) in enumerate(runs):
            base = mh.ACGT[i % 4]
            mid = np.full(run, base, np.uint8)
            if dinuc:
                mid = np.tile(np.array([base, mh.ACGT[(i + 1) % 4]], np.uint8), (run + 1) // 2)[:run]
            l = mh.ACGT[rng.integers(0, 4, 150)]; r = mh.ACGT[rng.integers(0, 4, 150)]
            if l[-1] == base: l[-1] = mh.ACGT[(i + 1) % 4]
            if r[0] == mid[-1]: r[0] = mh.ACGT[(i + 2) % 4] if mh.ACGT[(i + 2) % 4] != mid[-1] else mh.ACGT[(i + 3) % 4]
            txps.append(np.concatenate([l, mid, r])); names.append("run%d_%d%s" % (run, i, "d" if dinuc else "")); spots.append((150, run))
        d = mh.subdir(tmp_root, "runs_k%d" % k)
        fa = os.path.join(d, "t.fa")
        synth.write_fasta(fa, names, txps)
        idx = mh.build(fa, os.path.join(d, "idx"), k, "dense", threads=2)
        r1, r2 = [], []
        for t, (st, run) in zip(txps, spots):
            for back in list(range(0, 8)) + [17, 30]:
                a0 = st - back
                a = t[a0:a0 + 100].copy()
                b0 = min(len(t) - 100, a0 + 120)
                b = mh.COMP[t[b0:b0 + 100][::-1]]
                if back % 5 == 4:                               # a substitution right behind the run
                    p = min(99, back + run + 3)
                    a[p] = mh.ACGT[(np.searchsorted(mh.ACGT, a[p]) + 1) % 4]
                if back in (3, 6, 30):                          # ... and an N in the flank: the run in a read that is not clean
                    a[0] = ord("N")
                if back in (2, 5, 17):                          # ... or right in front of the run: the walk starts again on the run's first base
                    a[back - 1] = ord("N")
                if back % 2:
                    a, b = b, a
                r1.append(a.tobytes()); r2.append(b.tobytes())
        t = txps[-1]
        r1.append(b"A" * 100); r2.append(b"T" * 100)
        r1.append(b"A" * k + t[:100 - k].tobytes()); r2.append(b"C" * (k - 1) + t[:101 - k].tobytes())
        return {"fasta": fa, "idx": idx, "reads1": r1, "reads2": r2}
    return mh.once(("run_reads", k), make)


def fuzz_reads(text, offsets, n, seed, max_len, k):
    """test_gpu_parity._fuzz_reads with its shortest ordinary read relative to k: fragments of the indexed transcripts with substitutions,
    indels, N's, lower case, random tails and ragged lengths (15 % of them 0 .. max_len, the others max(k, max_len // 3) .. max_len)"""
    rng = np.random.default_rng(seed)
    lens = np.diff(np.append(offsets, text.size)) - 1
    ok = np.nonzero(lens >= 300)[0]
    acgt = np.frombuffer(b"ACGT", np.uint8)
    r1, r2 = [], []
    for i in range(n):
        t = ok[rng.integers(0, ok.size)]
        fl = int(rng.integers(60, min(400, lens[t])))
        st = int(rng.integers(0, lens[t] - fl + 1))
        frag = text[offsets[t] + st: offsets[t] + st + fl].copy()
        mates = []
        for m in range(2):
            L = int(rng.integers(0, max_len + 1)) if rng.random() < 0.15 else int(rng.integers(max(k, max_len // 3), max_len + 1))
            seq = frag[:L].copy() if m == 0 else mh.COMP[frag[::-1][:L]].copy()
            kind = rng.random()
            if seq.size and kind < 0.5:
                w = rng.random(seq.size) < 0.015
                seq[w] = rng.choice(acgt, int(w.sum()))
            if seq.size > 40 and 0.3 < kind < 0.6:
                p = int(rng.integers(5, seq.size - 5))
                seq = np.delete(seq, p) if rng.random() < 0.5 else np.insert(seq, p, rng.choice(acgt))
            if seq.size and rng.random() < 0.1:
                seq[rng.integers(0, seq.size)] = ord("N")
            if seq.size and rng.random() < 0.1:
                seq = np.frombuffer(seq.tobytes().lower(), np.uint8).copy()
            if seq.size > 50 and rng.random() < 0.05:
                seq[-20:] = rng.choice(acgt, 20)
            mates.append(seq[:max_len].tobytes())
        if rng.random() < 0.5:
            mates.reverse()
        r1.append(mates[0]); r2.append(mates[1])
    return r1, r2


# ---- the check that does not go through the oracle

def truth_pairs(tmp_root, n=2000, seed=99):
    """n error-free pairs of 2 x 100 characters off small_txome.  -> (q1, o, q2, o, truth); truth[i] = (sequence of the transcript the
    pair was cut from, where mate 1 lies in it, mate 1 forward?, where mate 2 lies, mate 2 forward?), the positions found by searching the
    transcript for the mate's characters (or their reverse complement)"""
    def make():
        from rapmap_amd import synth
        txps = [t for t in small_txome(tmp_root)["txps"] if t.size >= 400]
        s1, s2, off, where = synth.make_reads(txps, n, seed=seed, read_len=100, err=0.0)
        truth = []
        for i in range(n):
            t = txps[int(where[i, 0])].tobytes()
            sides = []
            for s in (s1, s2):
                r = s[off[i]:off[i + 1]].tobytes()
                rc = mh.COMP[np.frombuffer(r, np.uint8)[::-1]].tobytes()
                occ = {True: _occurrences(t, r), False: _occurrences(t, rc)}
                sides.append(occ)
            assert int(where[i, 1]) in sides[0][True] or int(where[i, 1]) in sides[1][True]
            truth.append((t, sides[0], sides[1]))
        return s1, off, s2, off, truth
    return mh.once(("truth_pairs", n, seed), make)


def _occurrences(t, r):
    out, p = set(), t.find(r)
    while p >= 0:
        out.add(p)
        p = t.find(r, p + 1)
    return out


def truth_check(hit_offsets, hits, truth, txp_seqs):
    """Every error-free pair's own transcript and position is among its hits: a paired hit on a transcript with the characters of the one
    the pair was cut from (txp_seqs[tid]: the index's transcripts as bytes), mate 1 and mate 2 where, and on the strand on which, a plain
    search of that transcript finds them.  Nothing here goes through the oracle or the index's suffix array."""
    missing = []
    for i, (t, occ1, occ2) in enumerate(truth):
        found = False
        for h in hits[hit_offsets[i]:hit_offsets[i + 1]]:
            if txp_seqs[int(h["tid"])] != t or h["mate_status"] != 3:       # 3: PE_PAIRED
                continue
            if int(h["pos"]) in occ1[bool(h["fwd"])] and int(h["mate_pos"]) in occ2[bool(h["mate_is_fwd"])]:
                found = True
                break
        if not found:
            missing.append(i)
    assert not missing, "%d of %d error-free pairs lack their true transcript and position, first: pair %d" % (len(missing), len(truth), missing[0])


def txp_seqs_of(idx):
    text, offsets = index_text(idx)
    ends = np.append(offsets[1:], text.size) - 1
    return [text[a:b].tobytes() for a, b in zip(offsets, ends)]


# ---- the lane emulation's own report of what the pair / lean kernels took (QM_EMU_LEAN_STATS=1, on stderr)

def emu_left(err_text):
    """{"pair": reads the pair kernel left in its fused pass, "lean": reads the lean kernel left after both of its passes} from what
    one emulated paired call printed"""
    import re
    out = {}
    m = re.search(r"pair kernel \(pass 0\) took (\d+) of (\d+) reads", err_text)
    if m:
        out["pair"] = int(m.group(2)) - int(m.group(1))
    m = re.search(r"lean kernel took (\d+) of (\d+) reads", err_text)
    if m:
        out["lean"] = int(m.group(2)) - int(m.group(1))
    m = re.search(r"N-aware pass over (\d+) reads, (\d+) marked again", err_text)
    if m:
        out["lean_first_pass"], out["lean_after_n_pass"] = int(m.group(1)), int(m.group(2))
    return out
