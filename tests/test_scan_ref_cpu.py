"""CPU: tests/scan_ref.py (the checker of tests/test_scan_compact_gpu.py) on literals written out by hand."""
import numpy as np

import scan_ref as R


def _eq(got, want, shape):
    got = np.asarray(got)
    assert got.dtype == np.int64 and got.shape == shape, (got.dtype, got.shape)
    assert got.tolist() == want


def test_pack_infos_empty():
    pi, total = R.pack_infos_from_counts([])
    _eq(pi, [], (0, 2))
    assert total == 0 and isinstance(total, int)


def test_pack_infos_all_zero():
    pi, total = R.pack_infos_from_counts([0, 0, 0])
    _eq(pi, [[0, 0], [0, 0], [0, 0]], (3, 2))
    assert total == 0


def test_pack_infos_docs_literal():
    """the literal of the pack_ops documentation (also tests/test_pack_ops_gpu.py::test_reference_known_answers)"""
    pi, total = R.pack_infos_from_counts(np.array([4, 1, 5, 3], np.int32))
    _eq(pi, [[0, 4], [4, 1], [5, 5], [10, 3]], (4, 2))
    assert total == 13


def test_pack_infos_beyond_32_bits():
    pi, total = R.pack_infos_from_counts([2 ** 32, 0, 2 ** 33 + 1, 7])
    _eq(pi, [[0, 2 ** 32], [2 ** 32, 0], [2 ** 32, 2 ** 33 + 1], [3 * 2 ** 32 + 1, 7]], (4, 2))
    assert total == 3 * 2 ** 32 + 8


def test_compact_empty():
    begin_all, idx, pi, totals = R.compact_packs([])
    _eq(begin_all, [], (0,))
    _eq(idx, [], (0,))
    _eq(pi, [], (0, 2))
    assert totals == (0, 0)


def test_compact_all_zero():
    begin_all, idx, pi, totals = R.compact_packs([0, 0, 0, 0], tag=[9, 8, 7, 6])
    _eq(begin_all, [0, 0, 0, 0], (4,))
    _eq(idx, [], (0,))
    _eq(pi, [], (0, 2))
    assert totals == (0, 0)


def test_compact_docs_literal():
    begin_all, idx, pi, totals = R.compact_packs([4, 1, 5, 3])
    _eq(begin_all, [0, 4, 5, 10], (4,))
    _eq(idx, [0, 1, 2, 3], (4,))
    _eq(pi, [[0, 4], [4, 1], [5, 5], [10, 3]], (4, 2))
    assert totals == (13, 4)


def test_compact_with_holes():
    begin_all, idx, pi, totals = R.compact_packs([0, 2, 0, 0, 3, 1, 0])
    _eq(begin_all, [0, 0, 2, 2, 2, 5, 6], (7,))
    _eq(idx, [1, 4, 5], (3,))
    _eq(pi, [[0, 2], [2, 3], [5, 1]], (3, 2))
    assert totals == (6, 3)


def test_compact_with_tags():
    begin_all, idx, pi, totals = R.compact_packs([0, 2, 0, 0, 3, 1, 0], tag=[70, 60, 50, 40, 30, 20, 10])
    _eq(begin_all, [0, 0, 2, 2, 2, 5, 6], (7,))
    _eq(idx, [60, 30, 20], (3,))
    _eq(pi, [[0, 2], [2, 3], [5, 1]], (3, 2))
    assert totals == (6, 3)
