"""The oracle's restatements against the REFERENCE ITSELF, for the pieces of the path whose own source files compile in this
image (oracle/Makefile.ref -> oracle/_ref/libqm_ref.so, built from /root/reference in place; see oracle/ref_harness.cpp):
ksw2pp's KSW2Aligner + ksw_extz2_sse (row a17), the Kmer<32,1> codec (a1), boomphf::mphf load + lookup (a3) and rank9b (a8).
This is what pins those four restatements; the collector / searcher / hit manager templates cannot be compiled here (they
include the un-vendored cereal) and stay corroborated by the reference's SAM fixtures only.

Where oracle/_ref cannot be built (no reference tree on the machine), every question goes to the reference's recorded answers
under tests/golden/reference_answers/ instead (answers() below); where it is built, the live answers must still equal the record.
A question about a file our own code writes records that file's SHA-256 too: the recorded answers hold for those bytes only."""
import ctypes as C
import os
import tarfile

import numpy as np
import pytest

from conftest import GOLD
from ref_answers import answers, load_ref, sha256

@pytest.fixture(scope="module")
def ref():
    """the live harness library with its signatures, or None: the tests then read the recorded answers"""
    L = load_ref()
    if L is None:
        return None
    L.ref_ksw_extension.restype = C.c_int
    L.ref_ksw_extension.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int] + [C.c_int] * 5
    L.ref_kmer.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
    L.ref_mphf_load.restype = C.c_void_p; L.ref_mphf_load.argtypes = [C.c_char_p]
    L.ref_mphf_lookup.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.ref_mphf_free.argtypes = [C.c_void_p]
    L.ref_rank_create.restype = C.c_void_p; L.ref_rank_create.argtypes = [C.c_void_p, C.c_uint64]
    L.ref_rank_query.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.ref_rank_free.argtypes = [C.c_void_p]
    return L


@pytest.fixture(scope="module")
def ref_index(tmp_path_factory):
    d = tmp_path_factory.mktemp("ref_index_o")
    with tarfile.open(os.path.join(GOLD, "sample_data", "ref_index.tar.gz")) as t:
        t.extractall(d)
    return {"dense": str(d / "dense"), "perfect": str(d / "perfect")}


SCHEMES = [(2, -4, 4, 2, 15), (2, -4, 4, 2, 5), (1, -1, 1, 1, 15), (2, -6, 5, 3, 33), (2, -4, 4, 2, 0), (4, -4, 6, 2, 20),
           (2, -4, 4, 2, 34), (2, -4, 4, 2, 64), (1, -1, 1, 1, 97), (2, -4, 4, 2, 150), (2, -4, 4, 2, 1000), (2, -4, 4, 2, -1),
           (1, 0, 25, 25, 15)]        # last: --mimicStrictBT2's scoring


@pytest.mark.parametrize("scheme", SCHEMES)
def test_ksw2_extension_score_equals_the_references(ref, oracle_mod, scheme):
    """the oracle's byte-exact emulation of ksw_extz2_sse41 (kswExtz2) == ksw2pp::KSW2Aligner(EXTENSION) as getAlnScore calls it"""
    from parity_cases import ksw_cases
    a, b, q_, e_, w = scheme
    ol = oracle_mod._lib()
    ol.qo_ksw_extz2.restype = C.c_int
    lut = np.frombuffer(b"ACGTN", dtype=np.uint8)
    cases = list(ksw_cases(777 + w, 600))
    score = answers("ksw2_extension_%d_%d_%d_%d_%d" % scheme, lambda L: {"score": [
        L.ref_ksw_extension(lut[q].tobytes(), len(q), lut[t].tobytes(), len(t), a, b, q_, e_, w) for q, t in cases]}, ref)["score"]
    bad = []
    for (q, t), want in zip(cases, score):
        got = ol.qo_ksw_extz2(len(q), q.ctypes.data_as(C.c_void_p), len(t), t.ctypes.data_as(C.c_void_p), a, b, q_, e_, w)
        if got != want:
            bad.append((len(q), len(t), int(want), got))
    assert not bad, "%d of 600 differ, first %r" % (len(bad), bad[:5])


def test_ksw2_long_and_dirty_inputs(ref, oracle_mod):
    """256-base queries, lower case and IUPAC characters (seq_nt4_table maps them to 4), every target length residue mod 16"""
    ol = oracle_mod._lib()
    ol.qo_ksw_extz2.restype = C.c_int
    rng = np.random.default_rng(5)
    nt4 = np.full(256, 4, np.uint8)
    for i, c in enumerate(b"ACGT"):
        nt4[c] = i; nt4[c + 32] = i
    nt4[:4] = [0, 1, 2, 3]
    alphabet = np.frombuffer(b"ACGTacgtNnRYKM", dtype=np.uint8)
    cases = []
    for it in range(300):
        ql = int(rng.integers(200, 257)); tl = min(276, ql + 20 - int(rng.integers(0, 17)))
        q = alphabet[rng.choice(len(alphabet), ql, p=[.2, .2, .2, .2] + [.02] * 10)]
        t = q[:tl].copy() if tl <= ql else np.concatenate([q, alphabet[rng.integers(0, 4, tl - ql)]])
        m = rng.random(tl) < 0.04
        t[m] = alphabet[rng.integers(0, 4, int(m.sum()))]
        cases.append((q, ql, t, tl, [15, 33, 60, -1][it % 4]))
    score = answers("ksw2_long_and_dirty", lambda L: {"score": [
        L.ref_ksw_extension(q.tobytes(), ql, t.tobytes(), tl, 2, -4, 4, 2, w) for q, ql, t, tl, w in cases]}, ref)["score"]
    for it, ((q, ql, t, tl, w), want) in enumerate(zip(cases, score)):
        qc = nt4[q]; tc = nt4[t]
        got = ol.qo_ksw_extz2(ql, qc.ctypes.data_as(C.c_void_p), tl, tc.ctypes.data_as(C.c_void_p), 2, -4, 4, 2, w)
        assert got == want, (it, ql, tl, w, want, got)


def test_kmer_codec_equals_the_references(ref, oracle_mod):
    """fromChars (incl. its partial word and return value at the first non-ACGT character), reverse complement, homopolymer"""
    ol = oracle_mod._lib()
    ol.qo_kmer_rc.restype = C.c_uint64; ol.qo_kmer_rc.argtypes = [C.c_uint64, C.c_int]
    ol.qo_kmer_homopolymer.argtypes = [C.c_uint64, C.c_int]
    rng = np.random.default_rng(11)
    alphabet = np.frombuffer(b"ACGTacgtNnUuRY$", dtype=np.uint8)
    cases = []
    for k in (31, 21, 5, 1):
        for it in range(3000):
            p = [.22] * 4 + [.02] * 4 + [.01] * 7
            p = np.array(p) / sum(p)
            cases.append((k, alphabet[rng.choice(len(alphabet), k, p=p)].tobytes() if it % 7 else bytes([b"ACGT"[it % 4]]) * k))

    def live(L):
        out = np.zeros((len(cases), 4), dtype=np.uint64)        # fromChars' return value, the word, its reverse complement, homopolymer
        for i, (k, s) in enumerate(cases):
            w, rc, hp = C.c_uint64(), C.c_uint64(), C.c_int()
            ok = L.ref_kmer(s, k, C.byref(w), C.byref(rc), C.byref(hp))
            out[i] = (ok, w.value, rc.value, hp.value)
        return {"kmer": out}
    rec = answers("kmer_codec", live, ref)["kmer"]
    for (k, s), (ok, w, rc, hp) in zip(cases, rec):
        ok, w, rc, hp = int(ok), int(w), int(rc), int(hp)
        v = C.c_int()
        ow = ol.qo_kmer_encode(s, len(s), k, C.byref(v))
        assert v.value == ok and ow == w, (k, s, ok, v.value, hex(w), hex(ow))
        if ok:
            assert ol.qo_kmer_rc(ow, k) == rc, (k, s)
            assert ol.qo_kmer_homopolymer(ow, k) == hp, (k, s)


def test_boophf_lookup_equals_the_references(ref, ref_index):
    """the numpy BooPHF model the emulation and the device walk are checked against (oracle/q5ph.py) == boomphf::mphf::lookup on
    the .bph the reference wrote: every indexed k-mer and 20 000 k-mers that are not in the index"""
    from oracle import q5, q5ph
    path = os.path.join(ref_index["perfect"], "hash_info.bph")
    boo = q5ph.BooPHF(path)
    ix = q5.load(ref_index["dense"])
    keys = np.ascontiguousarray(ix.hkeys, dtype=np.uint64)
    rng = np.random.default_rng(3)
    other = rng.integers(0, 1 << 62, 20000, dtype=np.uint64)
    allk = np.concatenate([keys, other])

    def live(L):
        h = L.ref_mphf_load(path.encode())
        assert h
        out = np.zeros(allk.size, dtype=np.uint64)
        L.ref_mphf_lookup(h, allk.ctypes.data, allk.size, out.ctypes.data)
        L.ref_mphf_free(h)
        return {"keys": allk, "lookup": out}
    a = answers("boophf_lookup", live, ref)
    assert np.array_equal(a["keys"], allk)
    out = a["lookup"]
    NOT_FOUND = (1 << 64) - 1                                # mphf::lookup returns ULLONG_MAX for a key the final hash does not hold
    mine = np.array([NOT_FOUND if (v := boo.lookup(int(x))) is None else v for x in allk], dtype=np.uint64)
    assert np.array_equal(out, mine)
    inidx = out[: keys.size]
    assert inidx.max() < keys.size and np.unique(inidx).size == keys.size          # a minimal perfect hash on its own keys


def test_rank_equals_the_references(ref, ref_index, oracle_mod):
    """rank9b::rank over rsd.bin (transcriptAtPosition, src/RapMapSAIndex.cpp:92-94) == the oracle's rank == the transcript whose
    text span holds the position (what the device's precomputed (tid, pos) table encodes)"""
    from oracle import oracle, q5
    raw = open(os.path.join(ref_index["dense"], "rsd.bin"), "rb").read()
    nbits = int(np.frombuffer(raw[:8], dtype="<u8")[0])
    bits = np.frombuffer(raw[8:], dtype=np.uint8).copy()
    ix = q5.load(ref_index["dense"])
    orc = oracle.Oracle(ix)
    pos = np.concatenate([np.arange(0, min(nbits, 3000)), np.random.default_rng(1).integers(0, nbits, 20000)]).astype(np.uint64)

    def live(L):
        h = L.ref_rank_create(bits.ctypes.data, nbits)
        out = np.zeros(pos.size, dtype=np.uint64)
        L.ref_rank_query(h, pos.ctypes.data, pos.size, out.ctypes.data)
        L.ref_rank_free(h)
        return {"pos": pos, "rank": out}
    a = answers("rank9b", live, ref)
    assert np.array_equal(a["pos"], pos)
    out = a["rank"]
    ol = oracle_mod._lib()
    mine = np.array([ol.qo_rank(orc.h, int(p)) for p in pos], dtype=np.uint64)
    assert np.array_equal(out, mine)
    offs = np.asarray(ix.txpOffsets, dtype=np.int64)
    text = np.asarray(ix.text)
    notsep = text[pos.astype(np.int64)] != ord("$")
    tid = np.searchsorted(offs, pos.astype(np.int64), side="right") - 1
    assert np.array_equal(out[notsep].astype(np.int64), tid[notsep])


def _spp(ref):
    ref.ref_spp_load.restype = C.c_void_p; ref.ref_spp_load.argtypes = [C.c_char_p]
    ref.ref_spp_size.restype = C.c_int64; ref.ref_spp_size.argtypes = [C.c_void_p]
    ref.ref_spp_dump.argtypes = [C.c_void_p] * 4
    ref.ref_spp_find.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    ref.ref_spp_free.argtypes = [C.c_void_p]
    ref.ref_xxh64.restype = C.c_uint64; ref.ref_xxh64.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    return ref


def _spp_dump(ref, path):
    h = ref.ref_spp_load(path.encode())
    assert h, "the reference's sparse_hash_map could not unserialize " + path
    n = ref.ref_spp_size(h)
    keys = np.zeros(n, dtype=np.uint64); lb = np.zeros(n, dtype=np.int32); ub = np.zeros(n, dtype=np.int32)
    ref.ref_spp_dump(h, keys.ctypes.data, lb.ctypes.data, ub.ctypes.data)
    return h, keys, lb, ub


def spp_answers(name, ref, path, probes=()):
    """what the reference's spp::sparse_hash_map says about the hash.bin at `path`: its records in container order (keys, lb,
    ub) and, for every probe array returned by probes(keys), find's (found, lb, ub).  Recorded with the file's SHA-256: the
    record answers for those bytes only."""
    data = open(path, "rb").read()

    def live(L):
        _spp(L)
        h, keys, lb, ub = _spp_dump(L, path)
        out = {"sha256": sha256(data), "keys": keys, "lb": lb, "ub": ub}
        try:
            for i, pr in enumerate(probes(keys) if probes else ()):
                pr = np.ascontiguousarray(pr, dtype=np.uint64)
                f = np.zeros(len(pr), dtype=np.uint8); fl = np.zeros(len(pr), dtype=np.int32); fu = np.zeros(len(pr), dtype=np.int32)
                L.ref_spp_find(h, pr.ctypes.data, len(pr), f.ctypes.data, fl.ctypes.data, fu.ctypes.data)
                out.update({"probe%d" % i: pr, "found%d" % i: f, "lb%d" % i: fl, "ub%d" % i: fu})
        finally:
            L.ref_spp_free(h)
        return out
    a = answers(name, live, ref)
    assert str(a["sha256"]) == str(sha256(data)), path + " is not the file the reference's container read"
    for i, pr in enumerate(probes(a["keys"]) if probes else ()):
        assert np.array_equal(a["probe%d" % i], pr)
    return a


def test_dense_hash_file_equals_the_references_container(ref, ref_index, oracle_mod):
    """hash.bin written by the reference, read back by the reference's own spp::sparse_hash_map::unserialize
    (include/sparsepp/spp.h:2355-2429 through include/SparseHashSerializer.hpp:31-47, as RapMapSAIndex::load does,
    src/RapMapSAIndex.cpp:67-76): the oracle's numpy reader (oracle/q5.py) must see the same key -> interval map, and the
    oracle's find (what every parity test's lookups go through) must answer like the container's find, for present and absent keys"""
    from oracle import q5
    from conftest import load_oracle
    d = ref_index["dense"]
    a = spp_answers("spp_reference_hash", ref, os.path.join(d, "hash.bin"), lambda keys: [np.concatenate(
        [keys, np.random.default_rng(3).integers(0, 1 << 62, 20000, dtype=np.uint64), keys ^ np.uint64(1)])])
    keys, lb, ub = a["keys"], a["lb"], a["ub"]
    k2, l2, u2 = q5.read_dense_hash(d)
    assert len(keys) == len(k2) == 18902
    o1 = np.argsort(keys); o2 = np.argsort(k2)
    assert np.array_equal(keys[o1], k2[o2]) and np.array_equal(lb[o1], l2[o2]) and np.array_equal(ub[o1], u2[o2])
    assert np.array_equal(keys, k2)                       # even the record order: the reader walks the file like the container
    ix, orc = load_oracle(d)
    probe, found, fl, fu = a["probe0"], a["found0"], a["lb0"], a["ub0"]
    assert found[: len(keys)].all() and not found[len(keys): len(keys) + 20000].any()
    ol = oracle_mod._lib()
    out = (C.c_int32 * 2)()
    for i in range(0, len(probe), 7):                    # every 7th probe through the oracle's own find
        got = ol.qo_hash_find(orc.h, int(probe[i]), out)
        assert bool(got) == bool(found[i])
        if got:
            assert (out[0], out[1]) == (fl[i], fu[i])


def test_our_hash_file_loads_in_the_references_container(ref, sample_data, lib_built):
    """hash.bin written by OUR index builder (rapmap_amd/csrc/qm_indexer.cpp) goes through the reference's unserialize, and the
    reference's find -- XXH64 + its own probing over the slots we chose -- returns every record: the file is a container the
    reference can use, not just the same map"""
    from oracle import q5
    d = sample_data["idx"]
    a = spp_answers("spp_our_hash", ref, os.path.join(d, "hash.bin"), lambda keys: [keys])
    keys, lb, ub = a["keys"], a["lb"], a["ub"]
    k2, l2, u2 = q5.read_dense_hash(d)
    assert np.array_equal(keys, k2) and np.array_equal(lb, l2) and np.array_equal(ub, u2) and len(keys) > 1000
    found, fl, fu = a["found0"], a["lb0"], a["ub0"]
    assert found.all() and np.array_equal(fl, lb) and np.array_equal(fu, ub)


def test_xxh64_equals_the_references(ref, lib_built):
    """the index builder's XXH64 (slot placement in hash.bin, duplicate filter) == src/xxhash.c, every length class of the
    algorithm (< 4, < 8, < 32, >= 32 bytes, unaligned tails), several seeds"""
    import rapmap_amd as ra
    L = ra.api.lib()
    L.qm_xxh64.restype = C.c_uint64; L.qm_xxh64.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    rng = np.random.default_rng(11)
    buf = rng.integers(0, 256, 4096, dtype=np.uint8)
    cases = [(shift, ln, seed) for ln in list(range(0, 100)) + [127, 128, 129, 1000, 4095] for seed in (0, 1, 0x9E3779B97F4A7C15)
             for shift in (0, 1, 3) if shift + ln <= buf.size]
    keys = rng.integers(0, 1 << 62, 5000, dtype=np.uint64)

    def live(R):
        _spp(R)
        return {"buf": np.array([R.ref_xxh64(buf.ctypes.data + shift, ln, seed) for shift, ln, seed in cases], dtype=np.uint64),
                "keys": np.array([R.ref_xxh64(keys[i:].ctypes.data, 8, 0) for i in range(len(keys))], dtype=np.uint64)}
    a = answers("xxh64", live, ref)
    for (shift, ln, seed), want in zip(cases, a["buf"]):
        assert L.qm_xxh64(buf.ctypes.data + shift, ln, seed) == int(want), (ln, seed, shift)
    assert len(a["buf"]) == len(cases) and len(a["keys"]) == len(keys)
    for i in range(len(keys)):
        assert L.qm_xxh64(keys[i:].ctypes.data, 8, 0) == int(a["keys"][i])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,compact", [("dense", False), ("perfect", False), ("perfect", True)])
def test_device_lookup_answers_like_the_references_container(ref, ref_index, lib_built, kind, compact):
    """the device's k-mer -> SA-interval lookup (bucket table built in HBM from hash.bin / from the -p files, or the BooPHF walk)
    against the REFERENCE's own container on the reference-written hash.bin: every indexed k-mer, given to the collector as
    a read of exactly k characters, must come back as the interval khash.find returns; random k-mers that the container does
    not hold (neither strand) must come back empty"""
    import rapmap_amd as ra
    k = 31
    def decode(words):
        sh = np.arange(k - 1, -1, -1, dtype=np.uint64) * np.uint64(2)
        return np.frombuffer(b"ACGT", dtype=np.uint8)[((words[:, None] >> sh[None, :]) & np.uint64(3)).astype(np.int64)]
    def rc(words):
        c = decode(words)[:, ::-1]
        m = np.zeros(256, dtype=np.uint64); m[ord("A")] = 3; m[ord("C")] = 2; m[ord("G")] = 1; m[ord("T")] = 0
        sh = np.arange(k - 1, -1, -1, dtype=np.uint64) * np.uint64(2)
        return (m[c] << sh[None, :]).sum(axis=1).astype(np.uint64)
    def probes(keys):
        absent = np.random.default_rng(5).integers(0, 1 << 62, 30000, dtype=np.uint64)
        return [absent, rc(absent)]
    a = spp_answers("spp_reference_hash_absent", ref, os.path.join(ref_index["dense"], "hash.bin"), probes)
    keys, lb, ub = a["keys"], a["lb"], a["ub"]
    absent = a["probe0"][(a["found0"] == 0) & (a["found1"] == 0)]
    words = np.concatenate([keys, absent])
    seq = decode(words).reshape(-1).copy(); off = np.arange(len(words) + 1, dtype=np.int64) * k
    qi = ra.QuasiIndex(ref_index[kind]); mp = ra.QuasiMapper(qi, 0, ph_compact=compact)
    found, ioff, ints = mp.collect_reads(seq, off)
    cnt = np.diff(ioff)
    assert not cnt[len(keys):].any() and not found[len(keys):].any()
    checked = 0
    for i in range(len(keys)):
        if not (0 < ub[i] - lb[i] < 1000):
            continue                                    # the collector does not record intervals of >= maxInterval suffixes
        g = ints[ioff[i]:ioff[i + 1]]
        fw = g[(g["query_rc"] == 0) & (g["query_pos"] == 0)]
        if len(fw) == 0:                               # homopolymer k-mers are never probed (include/SACollector.hpp:176-181)
            w = int(keys[i]); assert w in (0, (1 << 62) - 1) or len(set(decode(keys[i:i + 1])[0].tolist())) == 1, hex(w)
            continue
        assert len(fw) == 1 and (int(fw["begin"][0]), int(fw["end"][0]), int(fw["len"][0])) == (int(lb[i]), int(ub[i]), k), i
        checked += 1
    assert checked > 18000
    mp.close(); qi.close()


def _ref_fastx(ref, p1, p2=None):
    ref.ref_fastx_dump.restype = C.c_int64; ref.ref_fastx_dump.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]
    ref.ref_free.argtypes = [C.c_void_p]
    out = C.c_void_p()
    n = ref.ref_fastx_dump(p1.encode(), p2.encode() if p2 else None, C.byref(out))
    try:
        return [l.split(b"\t") for l in C.string_at(out, n).split(b"\n")[:-1]]
    finally:
        ref.ref_free(out)


def _records_sha(recs):
    return sha256(b"\n".join(b"\t".join(r) for r in recs))


def fastx_answers(name, ref, *paths):
    """what the reference's FastxParser reads from these files: (number of records, SHA-256 of the records, one per line with
    their fields tab-joined), recorded with the SHA-256 of each file's decompressed content"""
    import gzip as gz

    def content(p):
        with (gz.open(p, "rb") if p.endswith(".gz") else open(p, "rb")) as f:
            return sha256(f.read())
    files = np.array([str(content(p)) for p in paths])

    def live(L):
        recs = _ref_fastx(L, *paths)
        return {"files": files, "n": len(recs), "records": _records_sha(recs)}
    a = answers(name, live, ref)
    assert np.array_equal(a["files"], files), "not the files the reference's parser read"
    return int(a["n"]), str(a["records"])


def assert_reads(name, ref, got, *paths):
    n, sha = fastx_answers(name, ref, *paths)
    assert len(got) == n and str(_records_sha(got)) == sha, (name, len(got), n)


def test_ingest_engine_reads_what_the_references_parser_reads(ref, lib_built, tmp_path):
    """the ingest engine (rapmap_amd/csrc/qm_ingest.cpp: chunk-parallel parse with record resync, gz blocks) against the
    REFERENCE's own fastx_parser::FastxParser<ReadPair / ReadSeq> (src/FastxParser.cpp over kseq, compiled in place) on the same
    files: the reference's sample reads (gz), a plain paired FASTQ cut into 3 kB chunks with qualities that start with '@'
    and '+', CRLF lines and ragged lengths, and a multi-line FASTA -- same records, same order, same sequences; our names
    are the whole header line, the reference's end at the first blank (where the SAM writer cuts ours, src/RapMapUtils.cpp:334-351)"""
    import random
    import gzip as gz
    import rapmap_amd as ra

    def ours(p1, p2, batch, threads):
        rd = ra.FastxReader(p1, p2, threads=threads)
        out = []
        for b in rd.chunks(batch):
            for i in range(b.n):
                rec = [bytes(b.names1[b.name_off1[i]:b.name_off1[i + 1]]).split(b" ")[0].split(b"\t")[0], bytes(b.seq1[b.off1[i]:b.off1[i + 1]])]
                if p2:
                    rec += [bytes(b.names2[b.name_off2[i]:b.name_off2[i + 1]]).split(b" ")[0].split(b"\t")[0], bytes(b.seq2[b.off2[i]:b.off2[i + 1]])]
                out.append(rec)
        rd.close()
        return out

    g1 = os.path.join(GOLD, "sample_data", "reads_1.fastq.gz"); g2 = os.path.join(GOLD, "sample_data", "reads_2.fastq.gz")
    got = ours(g1, g2, 777, 3)
    assert len(got) == 10000
    assert_reads("fastx_sample_pair", ref, got, g1, g2)
    assert_reads("fastx_sample_single", ref, ours(g1, None, 4096, 2), g1)
    rnd = random.Random(7)
    p1 = str(tmp_path / "a.fq"); p2 = str(tmp_path / "b.fq")
    with open(p1, "wb") as f1, open(p2, "wb") as f2:
        for i in range(20000):
            for f, nl in ((f1, b"\n"), (f2, b"\r\n" if i % 5 == 0 else b"\n")):
                L = rnd.choice([1, 30, 31, 100, 100, 250]) if i % 40 == 0 else 100
                s = "".join(rnd.choice("ACGTN") for _ in range(L)).encode()
                q = "".join(rnd.choice("@+I5#") for _ in range(L)).encode()
                nm = ("r%d desc text/%d" % (i * 7919, 1 + (f is f2))).encode()
                f.write(b"@" + nm + nl + s + nl + b"+" + nl + q + nl)
    os.environ["QM_INGEST_CHUNK"] = "3000"
    try:
        got = ours(p1, p2, 1000, 6)
    finally:
        del os.environ["QM_INGEST_CHUNK"]
    assert len(got) == 20000
    assert_reads("fastx_ragged_pair", ref, got, p1, p2)
    # the same pair as BGZF files (independent gzip members, inflated by helper threads side by side here; one multi-member gzip
    # stream to the reference's kseq / gzread)
    from util import write_bgzf
    b1 = str(tmp_path / "a.bgzf.fq.gz"); b2 = str(tmp_path / "b.bgzf.fq.gz")
    write_bgzf(b1, open(p1, "rb").read(), block=5000); write_bgzf(b2, open(p2, "rb").read(), block=65280)
    assert_reads("fastx_ragged_pair_bgzf", ref, ours(b1, b2, 3000, 4), b1, b2)
    assert ours(b1, b2, 3000, 4) == got
    fa = str(tmp_path / "t.fa.gz")
    with gz.open(fa, "wt") as f:
        for i in range(3000):
            sq = "".join(rnd.choice("ACGT") for _ in range(rnd.randint(1, 400)))
            f.write(">t%d gene=%d\n" % (i, i // 3))
            for j in range(0, len(sq), 60):
                f.write(sq[j:j + 60] + "\n")
    assert_reads("fastx_multiline_fasta", ref, ours(fa, None, 257, 4), fa)
