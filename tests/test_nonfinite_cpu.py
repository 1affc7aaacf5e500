"""The oracle side of the non-finite contract of test_nonfinite_gpu.py, and the fixed-point / fp64 choice of the kernels'
scales restated in Python (no GPU).

The GPU tests compare the kernels' non-finite masks with the oracle's; these tests pin that the oracle's masks are the right
ones: a NaN in dL/dy row i, column c reaches exactly the entries that row's corners touch at that column's level."""
import struct

import numpy as np
import pytest

from util import LOTD_CASES, lotd_inputs

PRIMES = np.array([1, 2654435761, 805459861, 3674653429, 2097192037, 1434869437, 2165219737], np.uint64)


def _touched(md, x, row, col):
    """param indices that column `col` of point `row` interpolates, computed here in numpy (Dense / Hash levels:
    lotd_cuda.h index functions, positions x (res - 2) + 0.5)"""
    D, F = md["n_dims_to_encode"], md["n_feat_per_pseudo_lvl"]
    q, f = divmod(col, F)
    lvl, cnt = md["map_levels"][q], md["map_cnt"][q]
    res = np.array(md["level_res_multidim"][lvl], np.int64)
    Fl, off = md["level_n_feats"][lvl], md["level_offsets"][lvl]
    v = x[row].astype(np.float64) * (res - 2).astype(np.float32) + 0.5
    pg = np.floor(v.astype(np.float32)).astype(np.int64)
    out = set()
    for k in range(1 << D):
        p = pg + np.array([(k >> d) & 1 for d in range(D)])
        if md["level_types"][lvl] == 0:                                            # Dense: first dim most significant
            idx = 0
            for d in range(D):
                idx = idx * int(res[d]) + int(p[d])
        else:                                                                      # Hash
            h = np.uint64(0)
            for d in range(D):
                h ^= (np.uint64(p[d]) * PRIMES[d]) & np.uint64(0xFFFFFFFF)
            idx = int(h) % md["level_sizes"][lvl]
        out.add(off + idx * Fl + cnt * F + f)
    return out


POISON = [(3, 0), (7, 5), (11, 15)]          # (row, column): first feature of level 0, second of level 2, last column


def test_oracle_nan_reaches_exactly_the_touched_entries(oracle):
    md_case = LOTD_CASES["ngp_small"]
    m = oracle.lotd_create_meta(*md_case)
    md = m.as_dict()
    x, p, g, v = lotd_inputs(md, 200, 4)
    gp = g.copy()
    want = set()
    for r, c in POISON:
        gp[r, c] = np.nan
        want |= _touched(md, x, r, c)
    # the numpy index computation agrees with the oracle's grid index (the corner lists the GPU tests count updates with)
    gi = oracle.lotd_grid_index(m, x)
    for r, c in POISON:
        assert set(gi[r, c].tolist()) == _touched(md, x, r, c)
    for accum_double in (True, False):
        dp = oracle.lotd_bwd_dparam(m, gp, x, p, accum_double=accum_double)
        assert set(np.nonzero(~np.isfinite(dp))[0].tolist()) == want
    # second order: a NaN in dL/dy row r column c, and (separately) a NaN in dL/d(dL/dx) row r: every column of row r
    dp2 = oracle.lotd_bwd_bwd_dparam(m, v, gp, x, p, accum_double=True)
    assert set(np.nonzero(~np.isfinite(dp2))[0].tolist()) == want
    vp = v.copy()
    vp[9, 1] = np.nan
    dp3 = oracle.lotd_bwd_bwd_dparam(m, vp, g, x, p, accum_double=True)
    want3 = set().union(*(_touched(md, x, 9, c) for c in range(md["n_encoded_dims"])))
    assert set(np.nonzero(~np.isfinite(dp3))[0].tolist()) == want3
    # dL/dx: the poisoned rows, all of their components
    _, j = oracle.lotd_fwd(m, x, p, need_dydx=True)
    bad = ~np.isfinite(oracle.lotd_bwd_dx(m, gp, j)).all(1)
    assert set(np.nonzero(bad)[0].tolist()) == {r for r, _ in POISON}


def test_oracle_nan_reaches_what_a_one_hot_gradient_reaches(oracle):
    """metas with VM / CP levels (no closed index form here): the entries a NaN in (row, column) reaches are those a finite
    one-hot dL/dy at (row, column) gives a non-zero gradient -- the oracle neither drops a non-finite update nor spreads it"""
    m = oracle.lotd_create_meta(*LOTD_CASES["mixed"])
    md = m.as_dict()
    x, p, g, v = lotd_inputs(md, 300, 5)
    E = md["n_encoded_dims"]
    for r, c in [(3, 0), (40, 9), (77, E - 1), (120, E // 2)]:
        gp = g.copy()
        gp[r, c] = np.nan
        onehot = np.zeros_like(g)
        onehot[r, c] = 1.0
        reach = np.nonzero(oracle.lotd_bwd_dparam(m, onehot, x, p, accum_double=True))[0]
        assert reach.size > 0
        nf = np.nonzero(~np.isfinite(oracle.lotd_bwd_dparam(m, gp, x, p, accum_double=True)))[0]
        assert np.array_equal(nf, reach), (r, c)


# ---- the kernels' choice between 64-bit fixed point and fp64, restated ----------------------------------------------
def _bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0] if not isinstance(v, int) else v


def _f(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


# These restate the device code and are checked only against themselves here: a change to the device scales must be made in
# both places.  They mirror lotd_pair.hip pair_fix_bits (the PairFix struct above it), the bound lambdas of k_pair_bin and the
# `gm` lambda of lotd.hip k_contract_dx_rowmajor, and the s_bound block of lotd_bin.hip k_cp_direct (k_vm_direct's differs only
# in its constants).  test_nonfinite_gpu.py checks the kernels themselves.
def pair_fix_bits(bits, sum_log2):
    """lotd_pair.hip pair_fix_bits: (fixed point on, scale exponent)"""
    on = bits < 0x7F800000
    e = max(bits >> 23, 1) - 126
    lim = min(62 - sum_log2, 50 - 6)
    return on, max(min(lim - e, 1000), -1000)


def bound_bits(*vals):
    """max |v| as float bits (k_pair_bin, k_contract_dx_rowmajor): NaN bits are above +inf's, so a NaN anywhere wins"""
    return max(_bits(float(v)) & 0x7FFFFFFF for v in vals)


def s_bound_fix(gmax, pmax, pts, second=False, vmax=0.0, res=(8, 8, 8), opt_fix=1):
    """lotd_bin.hip k_cp_direct (the s_bound block): (fixed point on, scale exponent) from the workgroup's own maxima"""
    with np.errstate(over="ignore", invalid="ignore"):          # fp32 products as on the device: inf / NaN bounds are the point
        B = np.float32(gmax) * np.float32(pmax) * np.float32(pmax)
        if second:
            B = B * np.float32(7.5) * np.float32(max(res)) * np.float32(vmax)
    bb = _bits(float(B))
    if not (opt_fix and bb != 0 and bb < 0x7F000000 and B >= np.float32(1e-30)):
        return False, None
    e = (bb >> 23) - 126
    lg = 0
    while (1 << lg) < pts:
        lg += 1
    sc = min(62 - lg - 1, 44) - e
    return (-1000 < sc < 1000), sc


NAN_PATTERNS = [0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0xFFC00000]


@pytest.mark.parametrize("sum_log2", [3 + 16, 3 + 20, 3 + 22])
def test_pair_fix_bits_choice(sum_log2):
    lim = min(62 - sum_log2, 44)
    for v in (1.0, 0.37, 3.0e-20, 7.5e30, _f(0x7F7FFFFF), 2.0 ** -126, _f(1), _f(0x007FFFFF), 0.0):
        on, sc = pair_fix_bits(_bits(v) & 0x7FFFFFFF, sum_log2)
        assert on, v
        # every update |u| <= max|g| < 2^e: |u| 2^sc < 2^lim, and the sum of 2^sum_log2 of them stays below 2^62
        assert abs(v) * 2.0 ** sc < 2.0 ** lim and abs(v) * 2.0 ** (sc + sum_log2) < 2.0 ** 62
        if v >= 2.0 ** -126:       # a normal bound: the resolution 2^-sc is max|g| 2^-(lim - 1) or finer
            assert 2.0 ** -sc <= abs(v) * 2.0 ** -(lim - 1)
    for bits in [0x7F800000] + NAN_PATTERNS:
        assert not pair_fix_bits(bits & 0x7FFFFFFF, sum_log2)[0], hex(bits)


def test_bound_of_two_features_lets_nan_win():
    """the bound of a (point, pseudo level) update takes the max of |g0|, |g1| in float bits: a NaN or inf in ONE feature switches
    the call to fp64.  fmaxf (np.fmax) returns the number when the other operand is NaN -- the bound would stay finite."""
    for a, b in [(np.nan, 0.5), (0.5, np.nan), (np.inf, 0.5), (-np.inf, 0.25), (np.nan, np.nan)]:
        assert not pair_fix_bits(bound_bits(a, b), 23)[0], (a, b)
    assert pair_fix_bits(bound_bits(float(np.fmax(np.float32(np.nan), np.float32(0.5))), 0.0), 23)[0]   # the bug it prevents
    assert bound_bits(-0.75, 0.5) == _bits(0.75)


def test_s_bound_choice():
    on, sc = s_bound_fix(1.0, 0.1, 4096)
    assert on and sc is not None
    for g in (np.nan, np.inf, -np.inf):
        assert not s_bound_fix(g, 0.1, 4096)[0]                  # non-finite bound: fp64
        assert not s_bound_fix(0.5, g, 4096)[0]                  # a non-finite table value (product levels)
        assert not s_bound_fix(0.5, 0.1, 4096, second=True, vmax=g)[0]
    assert not s_bound_fix(0.0, 0.1, 4096)[0]                    # zero bound: fp64 (exact zeros either way)
    assert not s_bound_fix(_f(0x00000100), 0.1, 4096)[0]         # subnormal gradients: bound below 1e-30, fp64
    assert not s_bound_fix(1e30, 1e5, 4096)[0]                   # bound >= 2^127: fp64
    assert not s_bound_fix(1.0, 0.1, 4096, opt_fix=0)[0]
    assert s_bound_fix(np.float32(3.0e38), 0.1, 4096)[0]         # max finite gradient, bound still < 2^127: fixed point
