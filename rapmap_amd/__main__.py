"""`python -m rapmap_amd quasiindex|quasimap ...` -- the reference's command line on the MI355X path.

Flag names, defaults and validation follow `rapmap quasiindex` (src/RapMapSAIndexer.cpp:821-927) and
`rapmap quasimap` (src/RapMapSAMapper.cpp:984-1189, validateOpts :911-954).  Options that the device path does
not implement (--recoverOrphans) are accepted by the parser and rejected, never silently ignored.  -c/--chaining is
accepted like the reference accepts it: on its own it changes nothing there either (MappingConfig::doChaining is set from
--selAln alone, src/RapMapSAMapper.cpp:182,410).
"""
import argparse
import os
import sys
import time

import numpy as np


def _quasiindex(argv):
    ap = argparse.ArgumentParser(prog="rapmap_amd quasiindex", description="RapMap Indexer (MI355X build)")
    ap.add_argument("-t", "--transcripts", required=True, help="The transcript file to be indexed")
    ap.add_argument("-i", "--index", required=True, help="The location where the index should be written")
    ap.add_argument("-k", "--klen", type=int, default=31, help="The length of k-mer to index (odd, <= 31)")
    ap.add_argument("-p", "--perfectHash", action="store_true", help="Use a perfect hash instead of dense hash (BooPHF)")
    ap.add_argument("-n", "--noClip", action="store_true", help="Don't clip poly-A tails from the ends of target sequences")
    ap.add_argument("--keepDuplicates", action="store_true", help="Retain and index exact sequence-level duplicates")
    ap.add_argument("-s", "--headerSep", default=None, help="Instead of a space or tab, break the header at the first occurrence of "
                    "(one of the characters of) this string, and name the transcript as the token before the first separator")
    ap.add_argument("-x", "--numThreads", type=int, default=4, help="Threads for the k-mer interval scan / perfect hash")
    a = ap.parse_args(argv)
    if a.klen % 2 == 0 or a.klen > 31 or a.klen < 1:
        sys.exit("K-mer length should be odd and <= 31 (RapMapSAIndexer.cpp:870-877)")
    import rapmap_amd as ra
    t = time.time()
    ra.build_index(a.transcripts, a.index, k=a.klen, no_clip_poly_a=a.noClip, keep_duplicates=a.keepDuplicates,
                   threads=a.numThreads, perfect_hash=a.perfectHash, header_sep=a.headerSep)
    print("[rapmap_amd] index written to %s (%.1fs)" % (a.index, time.time() - t), file=sys.stderr)


def _quasimap(argv):
    ap = argparse.ArgumentParser(prog="rapmap_amd quasimap", description="RapMap Mapper (MI355X build)")
    ap.add_argument("-i", "--index", required=True, help="The location of the quasiindex")
    ap.add_argument("-1", "--leftMates", default="", help="The location of the left paired-end reads")
    ap.add_argument("-2", "--rightMates", default="", help="The location of the right paired-end reads")
    ap.add_argument("-r", "--unmatedReads", default="", help="The location of single-end reads")
    ap.add_argument("-t", "--numThreads", type=int, default=16, help="host threads for read parsing and SAM formatting (the GPU does the mapping)")
    ap.add_argument("-m", "--maxNumHits", type=int, default=200, help="Reads mapping to more than this many loci are discarded")
    ap.add_argument("-o", "--output", default="", help="The output file (default: stdout)")
    ap.add_argument("-z", "--quasiCoverage", type=float, default=None)
    ap.add_argument("-n", "--noOutput", action="store_true", help="Don't write out any alignments (for speed testing purposes)")
    ap.add_argument("--noSensitive", action="store_true")
    ap.add_argument("--noStrictCheck", action="store_true")
    ap.add_argument("-f", "--fuzzyIntersection", action="store_true")
    ap.add_argument("-c", "--chaining", action="store_true")
    ap.add_argument("-x", "--compressed", action="store_true", help="Compress the output SAM file using zlib")
    ap.add_argument("-q", "--quiet", action="store_true")
    ap.add_argument("-u", "--writeUnmapped", action="store_true")
    ap.add_argument("--recoverOrphans", action="store_true")
    ap.add_argument("--noDovetail", action="store_true")
    ap.add_argument("--noOrphans", action="store_true")
    ap.add_argument("-s", "--selAln", action="store_true", help="Perform selective alignment to validate mapping hits")
    ap.add_argument("--go", type=int, default=4, help="[only with selAln]: gap open penalty")
    ap.add_argument("--ge", type=int, default=2, help="[only with selAln]: gap extend penalty")
    ap.add_argument("--mm", type=int, default=-4, help="[only with selAln]: mismatch penalty")
    ap.add_argument("--ma", type=int, default=2, help="[only with selAln]: match score")
    ap.add_argument("--dpBandwidth", type=int, default=15)
    ap.add_argument("--minScoreFrac", type=float, default=0.65)
    ap.add_argument("--consensusSlack", type=float, default=0.2)
    ap.add_argument("--hardFilter", action="store_true")
    ap.add_argument("--mimicBT2", action="store_true")
    ap.add_argument("--mimicStrictBT2", action="store_true")
    ap.add_argument("--maxMMPExtension", type=int, default=7)
    ap.add_argument("--device", type=int, default=0, help="GPU to use")
    ap.add_argument("--devices", default="", help="comma-separated GPUs to use, or 'all': the read batches are dealt round-robin to the devices "
                    "(each holds its own index replica), results come back in input order")
    ap.add_argument("--eqClasses", default="", metavar="FILE", help="write the equivalence classes of the run (the sets of transcripts the "
                    "fragments map to, with their counts) to FILE in the format of Salmon's eq_classes.txt; they are built on the GPU, "
                    "and with -n no hit leaves the device")
    ap.add_argument("--quant", default="", metavar="FILE", help="estimate transcript abundances on the GPU (the EM over the run's equivalence "
                    "classes, which are built on the device whether or not --eqClasses is given) and write them to FILE in the format of "
                    "Salmon's quant.sf; with -n no hit leaves the device")
    ap.add_argument("--quantMaxIter", type=int, default=10000, help="[only with quant]: iterations of the EM at the most")
    ap.add_argument("--quantRelTol", type=float, default=1e-2, help="[only with quant]: stop when no abundance changes by more than this fraction")
    ap.add_argument("--quantFragLenMean", type=float, default=0.0, metavar="F", help="[only with quant]: effective length = max(1, Length - F + 1); "
                    "the default 0 takes the transcript length itself.  The fragment-length distribution is NOT estimated from the mapped pairs")
    ap.add_argument("--quantFLD", action="store_true", help="[only with quant, paired-end reads]: learn the fragment-length distribution from the "
                    "run's uniquely and properly paired fragments on the GPU; effective length = Length + 1 - (mean of the fragment lengths "
                    "that fit the transcript); the distribution is written to FILE.flenDist.txt.  Not together with --quantFragLenMean")
    ap.add_argument("--quantGCBias", action="store_true", help="[only with quantFLD]: one round of fragment GC bias correction: the run's uniquely and "
                    "properly paired fragments are counted by the GC fraction of their window on the transcript (observed), the same count "
                    "over every window of every transcript under the run's fragment-length distribution is computed on the GPU (expected), "
                    "and a second estimate, started from the first, runs on effective lengths weighted by observed / expected; bins, "
                    "counts and ratios are written to FILE.gcBias.txt")
    ap.add_argument("--quantSeqBias", action="store_true", help="[only with quantFLD, not with quantGCBias]: one round of sequence-specific bias "
                    "correction: the nucleotide contexts (nine characters, three of them upstream) at the two ends of the run's uniquely and "
                    "properly paired fragments are counted (observed), the same contexts over every place of every transcript a fragment "
                    "could start or end at are counted on the GPU under the first estimate and the run's fragment-length distribution "
                    "(expected), and a second estimate, started from the first, runs on effective lengths weighted by observed / expected, "
                    "computed on the GPU; counts and ratios are written to FILE.seqBias.txt")
    ap.add_argument("--quantPosBias", action="store_true", help="[only with quantFLD, not with quantGCBias or quantSeqBias]: one round of positional bias "
                    "correction: where along their transcript the run's uniquely and properly paired fragments start and end is counted in 20 bins "
                    "per class of transcript length (observed), the same bins over every place of every transcript a fragment could start or end "
                    "at are counted on the GPU under the first estimate and the run's fragment-length distribution (expected), and a second "
                    "estimate, started from the first, runs on effective lengths weighted by observed / expected, computed on the GPU; counts "
                    "and ratios are written to FILE.posBias.txt")
    ap.add_argument("--quantVB", action="store_true", help="[only with quant]: the variational Bayes EM in place of the EM: a transcript's weight is "
                    "exp(digamma(abundance + prior)) / effective length; the bootstrap replicates of --numBootstraps use it as well")
    ap.add_argument("--quantVBPrior", type=float, default=1e-2, metavar="P", help="[only with quantVB]: the prior, per nucleotide: P x effective length "
                    "for every transcript")
    ap.add_argument("--quantPerTranscriptPrior", action="store_true", help="[only with quantVB]: the prior is P for every transcript")
    ap.add_argument("--numBootstraps", type=int, default=0, metavar="B", help="[only with quant]: B bootstrap replicates of the estimate on the GPU (the "
                    "class counts resampled, the EM run again per replicate, 64 replicates at a time), written to FILE.bootstraps.gz in the "
                    "layout of Salmon's bootstraps.gz: B x transcripts little-endian float64")
    ap.add_argument("--bootstrapSeed", type=int, default=0, metavar="S", help="[only with numBootstraps]: seed of the resampling")
    ap.add_argument("--libType", default="", metavar="T", help="the library type, named as Salmon's -l names it (IU ISF ISR OU OSF OSR MU MSF MSR for "
                    "paired-end reads, U SF SR for single-end reads, A for any): every hit's orientation is tallied on the GPU, and with "
                    "--eqClasses / --quant only the hits that are compatible with T go into the classes; the tallies are written to "
                    "FILE.lib_format_counts.json next to the first of those files.  A drops nothing and reports the type the run points to")
    ap.add_argument("--chunk", type=int, default=1 << 18, help="read pairs per GPU batch")
    a = ap.parse_args(argv)
    if a.numBootstraps and not a.quant:
        ap.error("--numBootstraps needs --quant")
    if a.numBootstraps < 0:
        ap.error("--numBootstraps must not be negative")
    if a.quantFLD and not a.quant:
        ap.error("--quantFLD needs --quant")
    if a.quantGCBias and not a.quantFLD:
        ap.error("--quantGCBias needs --quantFLD")
    if a.quantSeqBias and not a.quantFLD:
        ap.error("--quantSeqBias needs --quantFLD")
    if a.quantSeqBias and a.quantGCBias:
        ap.error("--quantSeqBias and --quantGCBias are two corrections of their own: the joint model is not there, give one of them")
    if a.quantPosBias and not a.quantFLD:
        ap.error("--quantPosBias needs --quantFLD")
    if a.quantPosBias and (a.quantGCBias or a.quantSeqBias):
        ap.error("--quantPosBias and %s are two corrections of their own: the joint model is not there, give one of them" % ("--quantGCBias" if a.quantGCBias else "--quantSeqBias"))
    if a.quantVB and not a.quant:
        ap.error("--quantVB needs --quant")
    if not (a.quantVBPrior >= 0 and a.quantVBPrior < float("inf")):
        ap.error("--quantVBPrior must be a non-negative number")
    if a.quantFLD and a.quantFragLenMean:
        ap.error("--quantFLD learns the fragment lengths from the run: not together with --quantFragLenMean")
    if a.quantFLD and not (a.leftMates and a.rightMates):
        ap.error("--quantFLD needs paired-end reads (-1 and -2)")
    lib_types = ("IU", "ISF", "ISR", "OU", "OSF", "OSR", "MU", "MSF", "MSR", "U", "SF", "SR", "A")       # rapmap_amd.LIB_TYPES
    if a.libType and a.libType not in lib_types:
        ap.error("--libType must be one of " + " ".join(lib_types))
    if a.libType in ("U", "SF", "SR") and a.leftMates and a.rightMates:
        ap.error("--libType %s is a single-end type: not with paired-end reads (-1 and -2)" % a.libType)
    if a.libType and a.libType not in ("U", "SF", "SR", "A") and not (a.leftMates and a.rightMates):
        ap.error("--libType %s is a paired-end type: it needs paired-end reads (-1 and -2)" % a.libType)

    paired = bool(a.leftMates and a.rightMates)
    single = bool(a.unmatedReads)
    # validateOpts (src/RapMapSAMapper.cpp:911-954, :1179-1189)
    if paired == single:
        sys.exit("You must provide either paired-end (-1 and -2) or single-end (-r) reads, and not both")
    zset = a.quasiCoverage is not None                     # TCLAP isSet(): the flag was given, whatever its value
    if not zset:
        a.quasiCoverage = 0.0
    if not (0.0 <= a.quasiCoverage <= 1.0):
        sys.exit("quasiCoverage must be in [0,1]")
    if a.recoverOrphans:
        sys.exit("--recoverOrphans is not implemented on the MI355X path")
    if zset and a.noSensitive:                             # src/RapMapSAMapper.cpp:1178-1181
        print("The --quasiCoverage option is set to %g, but the --noSensitive flag was also set. The former forbids the later. "
              "Enabling sensitive mode." % a.quasiCoverage, file=sys.stderr)
        a.noSensitive = False
    if a.chaining and not (a.selAln or a.mimicBT2 or a.mimicStrictBT2):
        print("--chaining without --selAln does not change the mapping (as in the reference: doChaining follows --selAln)", file=sys.stderr)

    import rapmap_amd as ra
    opts = ra.default_opts(sensitive=0 if a.noSensitive else 1, strict_check=0 if a.noStrictCheck else 1,
                           max_num_hits=a.maxNumHits, no_orphans=int(a.noOrphans), no_dovetail=int(a.noDovetail),
                           fuzzy=int(a.fuzzyIntersection), sel_aln=int(a.selAln), quasi_cov=a.quasiCoverage)
    # --selAln and what it implies (src/RapMapSAMapper.cpp:1124-1175)
    if a.mimicBT2 and a.mimicStrictBT2:
        sys.exit("Cannot set --mimicBT2 and --mimicStrictBT2 simultaneously.  Please choose one")
    if a.mimicBT2 or a.mimicStrictBT2:
        opts.sel_aln = 1
    if opts.sel_aln:
        opts.gap_open, opts.gap_extend, opts.mismatch_penalty, opts.match_score = a.go, a.ge, a.mm, a.ma
        opts.dp_bandwidth, opts.min_score_fraction, opts.consensus_slack = a.dpBandwidth, a.minScoreFrac, a.consensusSlack
        opts.hard_filter, opts.max_mmp_extension = int(a.hardFilter), a.maxMMPExtension
        if a.mimicBT2 or a.mimicStrictBT2:
            opts.aln_policy = 2 if a.mimicStrictBT2 else 1
            opts.no_orphans = 1; opts.no_dovetail = 1; opts.consensus_slack = 0.35; opts.max_num_hits = 1000
        if a.mimicStrictBT2:
            opts.min_score_fraction = 0.8; opts.match_score = 1; opts.mismatch_penalty = 0; opts.gap_open = 25; opts.gap_extend = 25
    if a.devices:
        if a.devices == "all":
            import ctypes as _C
            nd = _C.c_int(0)
            hip = _C.CDLL("libamdhip64.so")
            if hip.hipGetDeviceCount(_C.byref(nd)) != 0 or nd.value <= 0:
                sys.exit("no HIP device visible")
            devices = list(range(nd.value))
        else:
            try:
                devices = [int(x) for x in a.devices.split(",") if x != ""]
            except ValueError:
                sys.exit("--devices takes a comma-separated list of device numbers, or 'all'")
            if not devices:
                sys.exit("--devices: no device given")
    else:
        devices = [a.device]
    # pinned memory for the stream's slots (every device of the run has its own), pinned in the background while the index is
    # opened and uploaded
    ra.reserve_stream_memory((1280 << 20) * len(devices))
    qi = ra.QuasiIndex(a.index)
    log = (lambda *x: None) if a.quiet else (lambda *x: print(*x, file=sys.stderr, flush=True))
    out = None
    direct_fd = None
    if not a.noOutput:
        out = open(a.output, "wb") if a.output else sys.stdout.buffer
        out.flush()
        try:
            direct_fd = out.fileno()
        except (OSError, ValueError, AttributeError):
            direct_fd = None                                 # a stdout that is not a descriptor: text goes through Python
    # header and records go from the library straight to the descriptor; -x: as gzip members compressed by the formatter's
    # workers (the reference wraps its output stream in a zlib compressor, src/RapMapSAMapper.cpp:832-833)
    writer = None
    if direct_fd is not None:
        writer = ra.SamWriter(qi, direct_fd, max_num_hits=opts.max_num_hits, threads=max(1, a.numThreads), gzip=bool(a.compressed))
        writer.header()
    elif out is not None:
        if a.compressed:
            import gzip
            out = gzip.GzipFile(fileobj=out, mode="wb")
        out.write(ra.sam_header_text(qi))
    tot = {"numReads": 0, "totHits": 0, "peHits": 0, "seHits": 0, "tooManyHits": 0}
    t0 = time.time()
    gpu_ms = 0.0
    nthr = max(1, a.numThreads)
    # ingest, mapping and result download are the library's pipelined stream (qm_stream_*): a reader thread parses the next
    # batch into pinned memory while two device contexts map the previous ones; SAM text (qm_sam_*) is formatted here from
    # the batch's pinned arrays.  -t sets the reader's / the formatter's worker count.
    if paired:
        files1, files2 = a.leftMates.split(","), a.rightMates.split(",")
        if len(files1) != len(files2):
            sys.exit("the number of left and right read files differs")
        pairs = list(zip(files1, files2))
    else:
        pairs = [(f, None) for f in a.unmatedReads.split(",")]
    # one context per device lives for the whole run: the index replica stays resident between the files of a multi-file run
    # (a stream's own contexts share it)
    keep = [ra.QuasiMapper(qi, d) for d in sorted(set(devices))]
    # --eqClasses: every stream folds its batches on the devices; the streams' merged tables (one per file) meet in this one
    classes = ra.EqClasses(keep[0]) if a.eqClasses or a.quant else None
    # --quantFLD: every stream folds its batches into fragment-length histograms as well; their sums (one per file) meet here
    fld_counts = np.zeros(ra.FLD_DEFAULT_MAX_LEN + 1, dtype=np.uint64) if a.quantFLD else None
    fld_stats = dict.fromkeys(ra.FLD_STATS, 0); fld_s = 0.0
    # --libType: every stream tallies its batches by orientation code and folds the compatible hits only; the tallies (one per file) meet here
    lib_counts = np.zeros(32, dtype=np.uint64) if a.libType else None
    # --quantGCBias: ... and sweeps them into observed GC counts; their sums (one per file) meet here
    gcb_obs = np.zeros(ra.GCB_BINS, dtype=np.uint64) if a.quantGCBias else None
    gcb_stats = dict.fromkeys(ra.GCB_STATS, 0); gcb_s = 0.0
    # --quantSeqBias: ... or into the observed counts of the end contexts
    sqb_obs = np.zeros((2, 9, 64), dtype=np.uint64) if a.quantSeqBias else None
    sqb_stats = dict.fromkeys(ra.SQB_STATS, 0); sqb_s = 0.0
    # --quantPosBias: ... or into the observed counts of the positions of the fragments' ends
    psb_obs = np.zeros((2, 5, 20), dtype=np.uint64) if a.quantPosBias else None
    psb_stats = dict.fromkeys(ra.PSB_STATS, 0); psb_s = 0.0
    for f1, f2 in pairs:
        os.environ.setdefault("QM_INGEST_PIN", "1")   # a whole-machine job with one ingest engine: its workers on the NUMA node that holds the files' pages
        st = ra.MappedStream(qi, f1, f2, opts=opts, device=devices, batch_units=a.chunk, threads=nthr, names=out is not None,
                             eq_classes=classes is not None, hits=out is not None or classes is None, frag_len_dist=a.quantFLD,
                             lib_type=a.libType or None, gc_bias=a.quantGCBias, seq_bias=a.quantSeqBias, pos_bias=a.quantPosBias)
        for b in st:
            gpu_ms += b.gpu_ms
            for kk in tot:
                tot[kk] += b.counters[kk]
            if out is not None:
                if writer is not None:
                    writer.put(b, b.hit_offsets, b.hits)       # formats now; the writer's thread writes while the next batch comes in
                else:
                    out.write(ra.sam_records_text(qi, b, b.hit_offsets, b.hits, max_num_hits=opts.max_num_hits, threads=nthr))
            if paired:
                log("saw %d reads : pe / read = %.4f : se / read = %.4f" % (
                    tot["numReads"], tot["peHits"] / max(1, tot["numReads"]), tot["seHits"] / max(1, tot["numReads"])))
        if classes is not None:
            classes.add_labels(*st.eq_classes())
        if a.libType:
            lib_counts += st.lib_counts()
        if a.quantFLD:
            c_, s_ = st.frag_len_dist()
            fld_counts += c_; fld_s += st.stats()["fld_fold_s"]
            for kk in fld_stats:
                fld_stats[kk] += s_[kk]
        if a.quantGCBias:
            c_, s_ = st.gc_bias()
            gcb_obs += c_; gcb_s += st.stats()["gcb_sweep_s"]
            for kk in gcb_stats:
                gcb_stats[kk] += s_[kk]
        if a.quantSeqBias:
            c_, s_ = st.seq_bias()
            sqb_obs += c_; sqb_s += st.stats()["sqb_sweep_s"]
            for kk in sqb_stats:
                sqb_stats[kk] += s_[kk]
        if a.quantPosBias:
            c_, s_ = st.pos_bias()
            psb_obs += c_; psb_s += st.stats()["psb_sweep_s"]
            for kk in psb_stats:
                psb_stats[kk] += s_[kk]
        log("stream: " + ", ".join("%s %.3f" % kv for kv in st.stats().items()))
        st.close()
    if a.libType:
        d = ra.lib_format_counts(lib_counts, a.libType)
        log("library type %s: %d hits (%s), %d units: %d without hits, %d compatible, %d dropped; the single-hit units point to %s" % (
            a.libType, d["hits"], ", ".join("%s %d" % kv for kv in d["hits_by_code"].items() if kv[1]), d["units"], d["unmapped_units"],
            d["kept_units"], d["dropped_units"], d["inferred_format"] or "no type"))
        if a.eqClasses or a.quant:
            ra.write_lib_format_counts((a.eqClasses or a.quant) + ".lib_format_counts.json", lib_counts, a.libType)
            log("wrote %s.lib_format_counts.json" % (a.eqClasses or a.quant))
    if classes is not None:
        if a.eqClasses:
            classes.write(a.eqClasses, qi.txp_names)
            log("wrote %d equivalence classes (%d fragments) to %s" % (classes.n_classes, classes.total, a.eqClasses))
        if a.quant:
            # --quant: the EM over the merged table where it lies; n_txps doubles come back
            lens = np.asarray(qi.txp_lens, dtype=np.int64)
            if a.quantFLD:
                eff = ra.eff_lens_from_counts(fld_counts, lens)
                ra.write_flen_dist(a.quant + ".flenDist.txt", fld_counts)
                log("fragment lengths: mean %g, %s, folded in %.3f ms; wrote %s.flenDist.txt" % (
                    ra.frag_len_mean(fld_counts), ", ".join("%s %d" % (kk, fld_stats[kk]) for kk in ra.FLD_STATS), fld_s * 1e3, a.quant))
                if not fld_stats["used"]:
                    log("no usable fragment (uniquely mapped, properly paired, 1 .. %d bases): effective length = length" % ra.FLD_DEFAULT_MAX_LEN)
            else:
                eff = np.maximum(1.0, lens.astype(np.float64) - a.quantFragLenMean + 1.0) if a.quantFragLenMean else np.maximum(1.0, lens.astype(np.float64))
            qn = ra.Quant(classes, qi.n_txps, eff)
            if a.quantVB:
                # --quantVB: the prior is built from the effective lengths that Quant was given
                qn.set_method("vbem", prior=a.quantVBPrior, per_transcript=a.quantPerTranscriptPrior)
            iters, rel = qn.run(max_iter=a.quantMaxIter, rel_tol=a.quantRelTol)
            if a.quantGCBias:
                # --quantGCBias: the expected matrix once on device 0, the effective lengths on the host, a second estimate over the
                # same table started from the first; what follows (quant.sf, the bootstrap) takes the second
                first = qn.fetch()
                gb = ra.GCBias(keep[0])
                H = gb.expect(fld_counts, qi.n_txps)
                expect_us = gb.stat()["last_expect_us"]; rank_us = gb.stat()["rank_build_us"]
                gb.close()
                eff, gc_exp, gc_ratio = ra.gc_eff_lens_from_counts(fld_counts, lens, H, first, gcb_obs)
                ra.write_gc_bias(a.quant + ".gcBias.txt", gcb_obs, gc_exp, gc_ratio)
                log("fragment GC: %s, swept in %.3f ms; expected counts in %.3f ms on the GPU (rank structure %.3f ms); ratios %g .. %g; wrote %s.gcBias.txt" % (
                    ", ".join("%s %d" % (kk, gcb_stats[kk]) for kk in ra.GCB_STATS), gcb_s * 1e3, expect_us / 1e3, rank_us / 1e3,
                    float(gc_ratio.min()), float(gc_ratio.max()), a.quant))
                qn.close()
                qn = ra.Quant(classes, qi.n_txps, eff)
                if a.quantVB:
                    qn.set_method("vbem", prior=a.quantVBPrior, per_transcript=a.quantPerTranscriptPrior)
                qn.set_start(first)
                it2, rel = qn.run(max_iter=a.quantMaxIter, rel_tol=a.quantRelTol)
                iters += it2
            if a.quantSeqBias:
                # --quantSeqBias: integer weights from the first estimate, the expected counts and the effective lengths on device 0,
                # a second estimate over the same table started from the first; what follows (quant.sf, the bootstrap) takes the second
                first = qn.fetch()
                sq_q, sq_k = ra.seq_bias_weights(first, lens, fld_counts)
                sb = ra.SeqBias(keep[0])
                sq_exp = sb.expect(fld_counts, qi.n_txps, sq_q)
                sq_ratio = ra.seq_bias_ratios(sqb_obs, sq_exp)
                eff = sb.eff_lens(fld_counts, qi.n_txps, sq_ratio)
                expect_us = sb.stat()["last_expect_us"]; efflen_us = sb.stat()["last_efflen_us"]
                sb.close()
                ra.write_seq_bias(a.quant + ".seqBias.txt", sqb_obs, sq_exp, sq_ratio)
                log("sequence bias: %s, swept in %.3f ms; weights 2^%d; expected counts in %.3f ms and effective lengths in %.3f ms on the GPU; ratios %g .. %g; "
                    "wrote %s.seqBias.txt" % (", ".join("%s %d" % (kk, sqb_stats[kk]) for kk in ra.SQB_STATS), sqb_s * 1e3, sq_k, expect_us / 1e3, efflen_us / 1e3,
                                              float(sq_ratio.min()), float(sq_ratio.max()), a.quant))
                qn.close()
                qn = ra.Quant(classes, qi.n_txps, eff)
                if a.quantVB:
                    qn.set_method("vbem", prior=a.quantVBPrior, per_transcript=a.quantPerTranscriptPrior)
                qn.set_start(first)
                it2, rel = qn.run(max_iter=a.quantMaxIter, rel_tol=a.quantRelTol)
                iters += it2
            if a.quantPosBias:
                # --quantPosBias: the steps of --quantSeqBias over the positional model: integer weights from the first estimate, the
                # expected counts and the effective lengths on device 0, a second estimate over the same table started from the first
                first = qn.fetch()
                ps_q, ps_k = ra.seq_bias_weights(first, lens, fld_counts)
                pb = ra.PosBias(keep[0])
                ps_exp = pb.expect(fld_counts, qi.n_txps, ps_q)
                ps_ratio = ra.pos_bias_ratios(psb_obs, ps_exp)
                eff = pb.eff_lens(fld_counts, qi.n_txps, ps_ratio)
                expect_us = pb.stat()["last_expect_us"]; efflen_us = pb.stat()["last_efflen_us"]
                pb.close()
                ra.write_pos_bias(a.quant + ".posBias.txt", psb_obs, ps_exp, ps_ratio)
                log("positional bias: %s, swept in %.3f ms; weights 2^%d; expected counts in %.3f ms and effective lengths in %.3f ms on the GPU; ratios %g .. %g; "
                    "wrote %s.posBias.txt" % (", ".join("%s %d" % (kk, psb_stats[kk]) for kk in ra.PSB_STATS), psb_s * 1e3, ps_k, expect_us / 1e3, efflen_us / 1e3,
                                              float(ps_ratio.min()), float(ps_ratio.max()), a.quant))
                qn.close()
                qn = ra.Quant(classes, qi.n_txps, eff)
                if a.quantVB:
                    qn.set_method("vbem", prior=a.quantVBPrior, per_transcript=a.quantPerTranscriptPrior)
                qn.set_start(first)
                it2, rel = qn.run(max_iter=a.quantMaxIter, rel_tol=a.quantRelTol)
                iters += it2
            ra.write_quant(a.quant, qi.txp_names, lens, eff, qn.fetch())
            what = "VBEM iterations, prior %g per %s" % (a.quantVBPrior, "transcript" if a.quantPerTranscriptPrior else "nucleotide") if a.quantVB else "EM iterations"
            log("wrote abundances of %d transcripts to %s (%d %s, %.3f ms on the GPU, last relative change %g)" % (
                qi.n_txps, a.quant, iters, what, qn.stat()["last_run_us"] / 1e3, rel))
            if a.numBootstraps:
                # --numBootstraps: batches of at most 64 replicates through first_rep, so that memory stays bounded
                import gzip
                us = 0
                with gzip.open(a.quant + ".bootstraps.gz", "wb") as f:
                    for first in range(0, a.numBootstraps, 64):
                        bs = ra.Bootstrap(qn, min(64, a.numBootstraps - first))
                        bs.resample(seed=a.bootstrapSeed, first_rep=first)
                        bs.run(max_iter=a.quantMaxIter, rel_tol=a.quantRelTol)
                        f.write(np.ascontiguousarray(bs.fetch(), dtype="<f8").tobytes())
                        st = bs.stat(); us += st["last_resample_us"] + st["last_run_us"]
                        bs.close()
                log("wrote %d bootstrap replicates to %s.bootstraps.gz (seed %d, %.3f ms on the GPU)" % (a.numBootstraps, a.quant, a.bootstrapSeed, us / 1e3))
            qn.close()
        classes.close()
    for k_ in keep:
        k_.close()
    if writer is not None:
        writer.close()
    if out is not None and out is not sys.stdout.buffer:
        out.close()
    log("Done mapping reads.")
    log("In total saw %d reads." % tot["numReads"])
    log("Final # hits per read = %g" % (tot["totHits"] / max(1, tot["numReads"])))       # RapMapSAMapper.cpp:892-893
    log("Elapsed time: %.3fs (GPU mapping %.3fs)" % (time.time() - t0, gpu_ms / 1e3))


def main():
    if len(sys.argv) < 2 or sys.argv[1] in ("-h", "--help"):
        print("usage: python -m rapmap_amd {quasiindex,quasimap} [options]\n"
              "  quasiindex  build a suffix array-based (SA) index\n"
              "  quasimap    map reads using the SA-based index (on an MI355X)")
        return
    if sys.argv[1] in ("-v", "--version"):
        import rapmap_amd as ra
        print("rapmap_amd", ra.api.lib().qm_version().decode())
        return
    cmd = sys.argv[1]
    if cmd == "quasiindex":
        _quasiindex(sys.argv[2:])
    elif cmd == "quasimap":
        _quasimap(sys.argv[2:])
    else:
        sys.exit("the command %s is not yet implemented" % cmd)       # src/RapMap.cpp:86-94


if __name__ == "__main__":
    main()
