"""numpy restatement of the device-wide exclusive scan (csrc/scan.h) and of the pack compaction (csrc/compact.h) -- the checker of
tests/test_scan_compact_gpu.py.  int64 throughout, nothing clever: ``np.cumsum`` and ``np.nonzero``; tests/test_scan_ref_cpu.py pins
both functions on literals written out by hand."""
import numpy as np


def _i64(counts):
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    assert (c >= 0).all(), "counts are lengths: never negative"
    return c


def pack_infos_from_counts(counts):
    """counts [n] -> (pack_infos int64 [n, 2] of (begin = exclusive cumsum, count), total python int): scan::pack_infos_from_counts"""
    c = _i64(counts)
    begin = np.cumsum(c, dtype=np.int64) - c
    return np.stack([begin, c], 1).reshape(-1, 2), int(c.sum(dtype=np.int64))


def compact_packs(counts, tag=None):
    """counts [n], tag int64 [n] | None -> (begin_all int64 [n], idx int64 [n_hit], pack_infos int64 [n_hit, 2], (sum, n_hit)):
    glue::compact_packs.  begin_all: the exclusive cumsum over EVERY pack; idx: the indices of the non-empty packs in ascending order
    (their tags when ``tag`` is given); pack_infos: (begin, count) of the non-empty packs in that order."""
    c = _i64(counts)
    begin_all = np.cumsum(c, dtype=np.int64) - c
    hit = np.nonzero(c)[0].astype(np.int64)
    idx = hit if tag is None else np.asarray(tag, dtype=np.int64).reshape(-1)[hit]
    pack_infos = np.stack([begin_all[hit], c[hit]], 1).reshape(-1, 2)
    return begin_all, idx, pack_infos, (int(c.sum(dtype=np.int64)), int(hit.shape[0]))
