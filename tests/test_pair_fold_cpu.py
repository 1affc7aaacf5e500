"""When the folded dL/dparam route of the pair path applies (host-side decision, no GPU needed)."""
import ctypes as C

import pytest

from util import LOTD_CASES


@pytest.fixture
def fold_bytes(hiplib):
    from nr3d_lib_amd import _hip as H
    return lambda m, n, ml: H.lib().nr3d_lotd_pair_fold_bytes(C.byref(m._cmeta()), n, ml)


def _meta(case):
    from nr3d_lib_amd.bindings import _lotd
    D, res, nf, types, T, smooth = LOTD_CASES[case]
    return _lotd.LoDMeta(D, res, nf, types, T, smooth)


def test_fold_applies_to_pair_metas(fold_bytes, hip_option):
    m = _meta("ngp_pair")
    n = 70001
    b = fold_bytes(m, n, m.n_levels - 1)
    # head (64 words + one ticket per bucket, rounded to 64 words) + one max per 256-point dL/dx workgroup
    assert b >= 4 * (64 + (n + 255) // 256) and b % 4 == 0
    assert 0 < fold_bytes(m, n, 1) <= b
    assert fold_bytes(m, n, -1) == 0 and fold_bytes(m, 0, 3) == 0
    hip_option("pair_fold", 0)
    assert fold_bytes(m, n, m.n_levels - 1) == 0


def test_fold_does_not_apply_elsewhere(fold_bytes):
    for case in ("dense_f8", "hash_4d", "dense_2d"):
        m = _meta(case)
        assert fold_bytes(m, 5000, m.n_levels - 1) == 0, case
