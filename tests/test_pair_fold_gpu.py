"""The folded dL/dparam route of the pair path (option pair_fold, default 1): a backward call with both gradients takes the
fixed-point scale and zeroed tickets from the dL/dx kernel, runs the replica plan inside the k_pair_direct launch and sums
split buckets and direct levels inside stage B.  Same scale, same plan, same summation order as the six-launch route
(pair_fold = 0): dL/dparam and dL/dx must be identical, bit for bit."""
import ctypes as C

import pytest
import torch

from util import LOTD_CASES

pytestmark = pytest.mark.gpu


def _c2_meta():
    from nr3d_lib_amd.bindings import _lotd
    from nr3d_lib_amd.models.grid_encodings.lotd import gen_ngp_cfg
    cfg = gen_ngp_cfg()
    return _lotd.LoDMeta(3, cfg["lod_res"], cfg["lod_n_feats"], cfg["lod_types"], cfg["hashmap_size"])


def _case_meta(case):
    from nr3d_lib_amd.bindings import _lotd
    D, res, nf, types, T, smooth = LOTD_CASES[case]
    return _lotd.LoDMeta(D, res, nf, types, T, smooth)


def _inputs(m, n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((n, 3), generator=g).clamp_(1e-6, 1 - 1e-6).to(dev)
    p = ((torch.rand((m.n_params,), generator=g) - 0.5) * 0.2).to(dev)
    dy = (torch.randn((n, m.n_encoded_dims), generator=g) * 0.01).to(dev)
    return x, p, dy


def _fold_bytes(m, n, max_level):
    from nr3d_lib_amd import _hip as H
    return H.lib().nr3d_lotd_pair_fold_bytes(C.byref(m._cmeta()), n, max_level)


def _bwd(m, x, p, dy, max_level=None):
    from nr3d_lib_amd.bindings import _lotd
    _, j = _lotd.lod_fwd(m, x, p, max_level=max_level, need_input_grad=True)
    return _lotd.lod_bwd(m, dy, x, p, j, max_level=max_level, need_input_grad=True, need_param_grad=True)


def _both(m, x, p, dy, hip_option, max_level=None):
    hip_option("pair_fold", 1)
    dx1, dp1 = _bwd(m, x, p, dy, max_level)
    dx1b, dp1b = _bwd(m, x, p, dy, max_level)
    hip_option("pair_fold", 0)
    dx0, dp0 = _bwd(m, x, p, dy, max_level)
    torch.cuda.synchronize()
    assert torch.equal(dp1, dp1b) and torch.equal(dx1, dx1b), "folded route not reproducible"
    assert torch.equal(dx1, dx0), "dL/dx differs between the routes"
    assert torch.equal(dp1, dp0), "dL/dparam differs between the routes"
    return dp1


@pytest.mark.parametrize("n", [1 << 20, (1 << 20) - 37])
def test_c2_meta_folded_equals_unfolded(dev, hip_option, n):
    m = _c2_meta()
    ml = m.n_levels - 1
    assert _fold_bytes(m, n, ml) > 0
    x, p, dy = _inputs(m, n, 1, dev)
    dp = _both(m, x, p, dy, hip_option)
    assert torch.isfinite(dp).all() and dp.abs().max() > 0


@pytest.mark.parametrize("case", ["ngp_pair", "ngp_small", "pair_f4"])
@pytest.mark.parametrize("half", [False, True])
def test_pair_cases_folded_equals_unfolded(dev, hip_option, case, half):
    m = _case_meta(case)
    x, p, dy = _inputs(m, 70001, 2, dev)
    if half:
        p, dy = p.half(), dy.half()
    _both(m, x, p, dy, hip_option)


@pytest.mark.parametrize("max_level", [1, 3])
def test_max_level_below_n_levels(dev, hip_option, max_level):
    m = _c2_meta()
    n = 300007
    assert _fold_bytes(m, n, max_level) > 0
    x, p, dy = _inputs(m, n, 3, dev)
    _both(m, x, p, dy, hip_option, max_level=max_level)


def test_largest_gradient_in_a_direct_level(dev, hip_option):
    """the fixed-point scale comes from a column of a level that k_pair_direct serves (levels 0 and 1 of C2)"""
    from nr3d_lib_amd import _hip
    m = _c2_meta()
    n = 200003
    assert _hip.lib().nr3d_lotd_pair_direct_levels(C.byref(m._cmeta()), n) >= 1
    x, p, dy = _inputs(m, n, 4, dev)
    dy[12345, 1] = 7.5
    dy[777, 2] = -6.0
    _both(m, x, p, dy, hip_option)


def test_largest_gradient_outside_the_served_columns(dev, hip_option):
    """with max_level = 4 the columns of levels 5.. are not served: their (huge) values must not set the scale"""
    m = _c2_meta()
    n = 200003
    x, p, dy = _inputs(m, n, 5, dev)
    dy[99, -1] = 1e6
    dy[100, 2 * 5] = -1e6
    dp = _both(m, x, p, dy, hip_option, max_level=4)
    # and the same call without the outliers gives the same levels 0..4 (the scale did not see them)
    dy[99, -1] = 0.0
    dy[100, 2 * 5] = 0.0
    hip_option("pair_fold", 1)
    _, dp2 = _bwd(m, x, p, dy, max_level=4)
    assert torch.equal(dp, dp2)


def test_two_streams_at_once(dev, hip_option):
    """two folded backward calls in flight on two streams: each equals its serial result"""
    m = _c2_meta()
    n = 1 << 19
    hip_option("pair_fold", 1)
    xa, pa, dya = _inputs(m, n, 6, dev)
    xb, pb, dyb = _inputs(m, n, 7, dev)
    ref_a, ref_b = _bwd(m, xa, pa, dya), _bwd(m, xb, pb, dyb)
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    outs = {}
    for _ in range(3):
        with torch.cuda.stream(sa):
            outs["a"] = _bwd(m, xa, pa, dya)
        with torch.cuda.stream(sb):
            outs["b"] = _bwd(m, xb, pb, dyb)
        torch.cuda.synchronize()
        for key, ref in (("a", ref_a), ("b", ref_b)):
            assert torch.equal(outs[key][0], ref[0]) and torch.equal(outs[key][1], ref[1]), key


def test_param_grad_only_keeps_the_old_route(dev, hip_option):
    """need_input_grad=False has no dL/dx kernel to hand anything over: the six-launch route, unchanged by the option"""
    from nr3d_lib_amd.bindings import _lotd
    m = _c2_meta()
    x, p, dy = _inputs(m, 100003, 8, dev)
    res = []
    for v in (1, 0):
        hip_option("pair_fold", v)
        res.append(_lotd.lod_bwd(m, dy, x, p, None, need_input_grad=False, need_param_grad=True)[1])
    torch.cuda.synchronize()
    assert torch.equal(res[0], res[1])
    full = _both(m, x, p, dy, hip_option)
    assert torch.equal(full, res[0])
