"""GPU: the `assign` rule of nr3d_lotd_bwd_dparam (include/nr3d_hip.h) on the routes that could not take an uninitialised
dL_dparam before ABI 20 -- corner records, a level range on the pair path, the atomic kernels, nothing to do -- through direct
calls of the entry.  n = 5003: one partial workgroup past a multiple of 1024, more than one point block per bucket."""
import ctypes as C

import pytest
import torch

from test_lotd_gpu import _setup
from util import assert_close

pytestmark = pytest.mark.gpu

N = 5003


def _dparam(s, out, n=N, min_level=0, assign=0, workspace=True):
    _lotd, m_ref, m, _, (xt, pt, gt, vt) = s
    from nr3d_lib_amd import _hip as H
    dev = xt.device
    ws, wsb = _lotd._dparam_workspace(m, n, dev, 1) if workspace and n else (None, 0)
    assert ws is not None or not (workspace and n)
    H.check(H.lib().nr3d_lotd_bwd_dparam(
        C.byref(m._cmeta()), H.ptr(m._dev(dev)), n, H.F32, H.ptr(gt), gt.stride(0), gt.stride(1), None, H.ptr(xt), H.F32, H.ptr(pt),
        None, None, 0, 1, min_level, m.n_levels, H.F32, assign, H.ptr(out), H.ptr(ws), wsb, None, H.stream_of(xt)))
    torch.cuda.synchronize()
    return out


def _nans(s):
    return torch.full_like(s[4][1], float("nan"))


@pytest.fixture(scope="module")
def ngp(oracle, dev):
    return _setup(oracle, dev, "ngp_small", n=N, seed=11)


def test_assign_on_corner_records(oracle, dev):
    """a meta of the record classes: the library's zero-fill and the caller's are the same sum (fp64 partial sums, no order)"""
    s = _setup(oracle, dev, "mixed", n=N, seed=11)
    want = _dparam(s, torch.zeros_like(s[4][1]))
    assert want.abs().max() > 0
    assert torch.equal(_dparam(s, _nans(s), assign=1), want)


def test_assign_with_a_level_range_on_the_pair_path(ngp):
    m = ngp[2]
    cut = m.n_levels // 2
    a = m.level_offsets[cut]
    want = _dparam(ngp, torch.zeros_like(ngp[4][1]), min_level=cut)
    got = _dparam(ngp, _nans(ngp), min_level=cut, assign=1)
    assert cut > 0 and not got[:a].any() and want[a:].abs().max() > 0
    assert torch.equal(got, want)


def test_assign_on_the_atomic_kernels(oracle, ngp):
    """no workspace: fp32 hardware atomics, whose order is free -- DESIGN section 2: 5e-5 of max |ref| per level"""
    _, m_ref, _, (x, p, g, v), _ = ngp
    got = _dparam(ngp, _nans(ngp), assign=1, workspace=False)
    assert not torch.isnan(got).any()
    assert_close(got, oracle.lotd_bwd_dparam(m_ref, g, x, p, accum_double=True), rel=5e-5, name="dL_dparam (atomics, assign)",
                 levels=m_ref)


def test_assign_with_no_points(ngp):
    assert not _dparam(ngp, _nans(ngp), n=0, assign=1).any()
