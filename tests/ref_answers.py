"""The reference's answers (test_oracle_ref.py, test_bigsa.py, test_big_index.py): live from the harness library oracle/_ref/libqm_ref.so
where it is built or can be built, else the record under tests/golden/reference_answers/.  No test functions here."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

from conftest import GOLD, ROOT

REF_SO = os.path.join(ROOT, "oracle", "_ref", "libqm_ref.so")
ANSWERS = os.path.join(GOLD, "reference_answers")


def answers(name, live, ref):
    """the reference's answers to one fixed set of questions, as a dict of arrays: live(ref) when the harness library is there
    (compared with the record, or written to it with QM_RECORD_REFERENCE=1), else the record tests/golden/reference_answers/<name>.npz"""
    path = os.path.join(ANSWERS, name + ".npz")
    if ref is None:
        assert os.path.exists(path), "no reference harness here and no recorded answers " + path
        with np.load(path) as z:
            return {k: z[k] for k in z.files}
    got = {k: np.asarray(v) for k, v in live(ref).items()}
    if os.environ.get("QM_RECORD_REFERENCE") == "1":
        os.makedirs(ANSWERS, exist_ok=True)
        np.savez_compressed(path, **got)
    else:
        with np.load(path) as z:
            assert sorted(z.files) == sorted(got) and all(np.array_equal(z[k], got[k]) for k in got), "live answers differ from " + path
    return got


def sha256(data):
    return np.array(hashlib.sha256(data).hexdigest())


def load_ref():
    """the harness library, built by oracle/Makefile.ref where the reference tree it names is present; None where it is not"""
    if not os.path.exists(REF_SO):
        if subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "-f", "Makefile.ref"], capture_output=True).returncode:
            return None
    return C.CDLL(REF_SO)


def check_spp64(L, blob, expect, name):
    """`blob` (a serialised spp::sparse_hash_map<int64_t, int64_t>) loads in the reference's container and holds exactly `expect`
    (L None: the container's recorded answers for the blob of that SHA-256)"""
    import tempfile
    keys = np.array(sorted(expect) + [max(expect) + 1, -5, 1 << 40], dtype=np.int64)

    def live(L):
        L.ref_spp64_load.restype = C.c_void_p; L.ref_spp64_load.argtypes = [C.c_char_p]
        L.ref_spp64_size.restype = C.c_int64; L.ref_spp64_size.argtypes = [C.c_void_p]
        L.ref_spp64_find.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.ref_spp64_free.argtypes = [C.c_void_p]
        with tempfile.NamedTemporaryFile(suffix=".spp") as f:
            f.write(blob); f.flush()
            h = L.ref_spp64_load(f.name.encode())
        assert h, name + ": the reference's container did not load the map"
        try:
            found = np.zeros(keys.size, dtype=np.uint8); val = np.zeros(keys.size, dtype=np.int64)
            L.ref_spp64_find(h, keys.ctypes.data, keys.size, found.ctypes.data, val.ctypes.data)
            return {"sha256": sha256(blob), "keys": keys, "size": L.ref_spp64_size(h), "found": found, "val": val}
        finally:
            L.ref_spp64_free(h)
    a = answers(name, live, L)
    assert str(a["sha256"]) == str(sha256(blob)) and np.array_equal(a["keys"], keys), "not the map the reference's container read"
    assert int(a["size"]) == len(expect), (name, int(a["size"]), len(expect))
    found, val = a["found"], a["val"]
    assert found[:-3].all() and not found[-3:].any(), (name, found.tolist())
    assert [int(v) for v in val[:-3]] == [expect[int(k)] for k in keys[:-3]], name + ": the values found are not the expected ones"
