"""Multi-GPU: one process per GPU, read pairs statically sharded, full index replica per GPU, and ONE
collective -- the sum of the HitCounters (include/RapMapUtils.hpp:208-216) -- after the last batch
(SURVEY.md section 8e).  torch.distributed is plumbing here: backend "nccl" is RCCL over xGMI on the
GPU box, "gloo" in the CPU tests."""
import numpy as np
import torch
import torch.distributed as dist

COUNTER_KEYS = ["peHits", "seHits", "totHits", "numReads", "tooManyHits", "mappedUnits"]


def shard_bounds(n, rank, world):
    """contiguous static split: shard g = units [g*n/W, (g+1)*n/W)"""
    return (n * rank) // world, (n * (rank + 1)) // world


def all_reduce_counters(counters, device):
    """dict of the six counters -> dict of their sums over all ranks (48 bytes on the wire)"""
    if not (dist.is_available() and dist.is_initialized()):
        # no process group (a plain one-process run): nothing to sum over -- and no tensor round trip through the device for it (0.5-0.8 ms of
        # host latency per call behind a 21 ms step, profiles/r06/timeline.sh)
        return {k: int(counters[k]) for k in COUNTER_KEYS}
    t = torch.tensor([int(counters[k]) for k in COUNTER_KEYS], dtype=torch.int64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)                # (also with ONE rank under torchrun: the collective library runs, the sum is the input)
    return dict(zip(COUNTER_KEYS, (int(x) for x in t.cpu())))


def all_reduce_frag_len_counts(counts, device):
    """a fragment-length histogram (FragLenDist.counts, MappedStream.frag_len_dist) -> its sum over all ranks: one int64 all_reduce
    over the bins (8 KB on the wire).  Without a process group the input comes back unchanged, as all_reduce_counters does for
    counters.  The sum goes into a histogram through FragLenDist.add_counts."""
    if not (dist.is_available() and dist.is_initialized()):
        return counts
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    t = torch.from_numpy(c.view(np.int64).copy()).to(device)    # (counts stay far below 2^63: the bits are the same either way)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t.cpu().numpy().view(np.uint64)


def all_reduce_gc_counts(obs, device):
    """the observed counts of the fragment GC bias model (GCBias.counts, MappedStream.gc_bias) -> their sum over all ranks: one int64
    all_reduce over the 25 bins (200 bytes on the wire).  Without a process group the input comes back unchanged.  The sum goes into an
    object through GCBias.add_counts."""
    if not (dist.is_available() and dist.is_initialized()):
        return obs
    c = np.ascontiguousarray(obs, dtype=np.uint64)
    t = torch.from_numpy(c.view(np.int64).copy()).to(device)    # (counts stay far below 2^63: the bits are the same either way)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t.cpu().numpy().view(np.uint64)


def all_reduce_seq_counts(obs, device):
    """the observed counts of the sequence-specific bias model (SeqBias.counts, MappedStream.seq_bias) -> their sum over all ranks, in
    the input's shape: one int64 all_reduce over the 1152 entries (9 KB on the wire).  Without a process group the input comes back
    unchanged.  The sum goes into an object through SeqBias.add_counts."""
    if not (dist.is_available() and dist.is_initialized()):
        return obs
    c = np.ascontiguousarray(obs, dtype=np.uint64)
    t = torch.from_numpy(c.view(np.int64).copy()).to(device)    # (counts stay far below 2^63: the bits are the same either way)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t.cpu().numpy().view(np.uint64)


def all_reduce_pos_counts(obs, device):
    """the observed counts of the positional bias model (PosBias.counts, MappedStream.pos_bias) -> their sum over all ranks, in the
    input's shape: one int64 all_reduce over the 200 entries (1 600 bytes on the wire).  Without a process group the input comes back
    unchanged.  The sum goes into an object through PosBias.add_counts."""
    if not (dist.is_available() and dist.is_initialized()):
        return obs
    c = np.ascontiguousarray(obs, dtype=np.uint64)
    t = torch.from_numpy(c.view(np.int64).copy()).to(device)    # (counts stay far below 2^63: the bits are the same either way)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t.cpu().numpy().view(np.uint64)


def all_reduce_lib_counts(counts, device):
    """the tallies of a library type (LibFormat.counts, MappedStream.lib_counts) -> their sum over all ranks: one int64 all_reduce over
    the 32 words (256 bytes on the wire).  Without a process group the input comes back unchanged.  The sum goes into an object through
    LibFormat.add_counts."""
    if not (dist.is_available() and dist.is_initialized()):
        return counts
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    t = torch.from_numpy(c.view(np.int64).copy()).to(device)    # (counts stay far below 2^63: the bits are the same either way)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t.cpu().numpy().view(np.uint64)


def merge_eq_classes(table, mapper=None):
    """Every rank's equivalence classes into every rank's table: the fetched tables are all-gathered and each rank folds the
    others' in through EqClasses.add_labels, counts as weights (the table's one merge primitive).  Without a process group the
    table is returned unchanged, as all_reduce_counters does for counters.  mapper: the rank's QuasiMapper (its device carries
    the collective's tensors under the nccl backend)."""
    if not (dist.is_available() and dist.is_initialized()):
        return table
    off, tids, cnt = table.fetch()
    mine = {"off": off, "tids": tids, "cnt": cnt}
    parts = [None] * dist.get_world_size()
    if mapper is not None and dist.get_backend() == "nccl":
        torch.cuda.set_device(mapper.device)                # all_gather_object moves its pickles through the current device
    dist.all_gather_object(parts, mine)
    me = dist.get_rank()
    for r, p in enumerate(parts):
        if r != me and len(p["cnt"]):
            table.add_labels(p["off"], p["tids"], p["cnt"])
    return table
