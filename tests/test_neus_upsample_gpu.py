"""The fused up-sampling stage (csrc/neus_upsample.hip) through bindings._neus_upsample.upsample_stage.

Values: `fine` against the float64 run of the restatement (tests/neus_coarse_ref.py) on the same float32 inputs.  The tolerance is
measured, not fixed: e_ref = max |float32 restatement - float64 restatement| on those inputs, and the kernel may be 4 e_ref plus one
ulp of the largest depth away -- it associates its products and sums as a tree where torch goes left to right, with an error bound
of the same order n 2^-24 either way.  The comparison needs a well-conditioned inverse CDF, which the parity cases assert: every
ray's float64 weight sum is at least 0.99.
Structure: `merged` and `order` are checked exactly on the kernel's own `fine`."""
import numpy as np
import pytest
import torch

import neus_coarse_ref as ref
from nr3d_lib_amd.bindings import _neus_upsample as U

pytestmark = pytest.mark.gpu


def sphere_rows(R, n, near=ref.NEAR, far=ref.FAR):
    """depth [R, n] uniform in [near, far] on the first R rays of a fan, sdf of the sphere there (float32, CPU)"""
    k = int(np.ceil(np.sqrt(R)))
    rays = ref.fan_rays(max(k, 2))
    o, v = rays['rays_o'][:R], rays['rays_d'][:R]
    depth = torch.linspace(near, far, n).expand(R, n).contiguous()
    sdf = (o[:, None, :] + v[:, None, :] * depth[..., None]).norm(dim=-1) - ref.RADIUS
    return depth, sdf.contiguous()


def run(dev, depth, sdf, u, inv_s, est):
    fine, merged, order = U.upsample_stage(depth.to(dev), sdf.to(dev), u.to(dev), inv_s, est)
    torch.cuda.synchronize()
    return fine.cpu(), merged.cpu(), order.cpu()


def check_structure(depth, fine, merged, order):
    R, n = depth.shape
    m = fine.shape[1]
    both = torch.cat([depth, fine], -1)
    assert merged.shape == order.shape == (R, n + m) and order.dtype == torch.int32
    assert torch.equal(merged, both.sort(dim=-1).values), "merged is not sort(cat([depth, fine])) bit for bit"
    assert torch.equal(order.long().sort(dim=-1).values, torch.arange(n + m).expand(R, n + m)), "order is not a permutation"
    assert torch.equal(both.gather(-1, order.long()), merged)
    tie = merged[:, 1:] == merged[:, :-1]
    assert not (tie & (order[:, :-1] >= n) & (order[:, 1:] < n)).any(), "a new depth precedes an equal boundary"
    assert not (tie & ((order[:, :-1] >= n) == (order[:, 1:] >= n)) & (order[:, :-1] > order[:, 1:])).any(), "equal values out of order"


def check_values(depth, sdf, u, inv_s, est, fine, need_mass=False):
    r32 = ref.stage(depth, sdf, u, inv_s, est, torch.float32)
    r64 = ref.stage(depth, sdf, u, inv_s, est, torch.float64)
    if need_mass:
        assert r64['wsum'].min().item() >= 0.99, f"precondition: weight sum {r64['wsum'].min().item()}"
    e_ref = (r32['fine'].double() - r64['fine']).abs().max().item()
    err = (fine.double() - r64['fine']).abs().max().item()
    ulp = float(np.spacing(np.float32(depth.abs().max().item())))
    print(f"n={depth.shape[1]} m={fine.shape[1]} inv_s={inv_s} est={est}: kernel {err:.3e}  e_ref {e_ref:.3e}  allowed {4 * e_ref + ulp:.3e}")
    assert torch.isfinite(fine).all()
    assert err <= 4 * e_ref + ulp
    return err, e_ref


@pytest.mark.parametrize("inv_s", [64, 128, 256, 512])
@pytest.mark.parametrize("est", [False, True])
@pytest.mark.parametrize("n,m", [(17, 9), (65, 65)])
def test_parity(dev, n, m, est, inv_s):
    depth, sdf = sphere_rows(64, n)
    u = ref.shared_u(m)
    fine, merged, order = run(dev, depth, sdf, u, float(inv_s), est)
    check_values(depth, sdf, u, float(inv_s), est, fine, need_mass=True)
    check_structure(depth, fine, merged, order)


@pytest.mark.parametrize("R,n,m", [(1, 17, 9), (130, 17, 9), (64, 2, 1), (64, 67, 33)])
@pytest.mark.parametrize("est", [False, True])
def test_shapes(dev, R, n, m, est):
    depth, sdf = sphere_rows(R, n)
    u = ref.shared_u(m)
    fine, merged, order = run(dev, depth, sdf, u, 64.0, est)
    assert fine.shape == (R, m)
    check_values(depth, sdf, u, 64.0, est, fine)
    check_structure(depth, fine, merged, order)


def test_max_row(dev):
    m = 65
    n = U.MAX_ROW - m
    assert U.MAX_ROW >= 1024
    depth, sdf = sphere_rows(5, n)
    u = ref.shared_u(m)
    fine, merged, order = run(dev, depth, sdf, u, 64.0, False)
    check_values(depth, sdf, u, 64.0, False, fine)
    check_structure(depth, fine, merged, order)
    depth, sdf = sphere_rows(5, n + 1)
    with pytest.raises(RuntimeError, match="MAX_ROW"):
        U.upsample_stage(depth.to(dev), sdf.to(dev), u.to(dev), 64.0, False)


@pytest.mark.parametrize("est", [False, True])
def test_per_ray_u(dev, est):
    R, n, m = 64, 65, 33
    depth, sdf = sphere_rows(R, n)
    g = torch.Generator().manual_seed(7)
    u = ((torch.arange(m) + torch.rand(R, m, generator=g)) / m).contiguous()          # stratified, hence sorted
    fine, merged, order = run(dev, depth, sdf, u, 128.0, est)
    check_values(depth, sdf, u, 128.0, est, fine)
    check_structure(depth, fine, merged, order)
    shared = run(dev, depth, sdf, u[0].contiguous(), 128.0, est)[0]
    assert torch.equal(shared[0], fine[0]) and not torch.equal(shared, fine)


@pytest.mark.parametrize("est", [False, True])
def test_missing_ray(dev, est):
    R, n, m = 3, 17, 9
    depth, _ = sphere_rows(R, n)
    sdf = (1.0 + 0.25 * (depth - 2.5).abs()).contiguous()                             # never below 1: every alpha is exactly 0
    fine, merged, order = run(dev, depth, sdf, ref.shared_u(m), 64.0, est)
    assert torch.equal(fine, depth[:, -1:].expand(R, m))
    assert torch.equal(merged[:, -(m + 1):], depth[:, -1:].expand(R, m + 1)) and torch.equal(merged[:, :n], depth)
    check_structure(depth, fine, merged, order)


@pytest.mark.parametrize("est", [False, True])
def test_zero_length_ray(dev, est):
    R, n, m = 4, 17, 9
    depth, sdf = sphere_rows(R, n, near=2.0, far=2.0)
    u = ref.shared_u(m)
    fine, merged, order = run(dev, depth, sdf, u, 64.0, est)
    assert torch.isfinite(fine).all() and torch.isfinite(merged).all()
    assert torch.equal(fine, ref.stage(depth, sdf, u, 64.0, est, torch.float32)['fine'])
    check_structure(depth, fine, merged, order)


def test_same_bytes_run_after_run(dev):
    depth, sdf = sphere_rows(130, 65)
    u = ref.shared_u(65)
    a, b = run(dev, depth, sdf, u, 256.0, True), run(dev, depth, sdf, u, 256.0, True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_argument_checks(dev):
    depth, sdf = sphere_rows(4, 17)
    d, s, u = depth.to(dev), sdf.to(dev), ref.shared_u(9).to(dev)
    with pytest.raises(RuntimeError, match="GPU only"):
        U.upsample_stage(depth, s, u, 64.0, False)
    with pytest.raises(RuntimeError, match="float32"):
        U.upsample_stage(d.double(), s, u, 64.0, False)
    with pytest.raises(RuntimeError, match="contiguous"):
        U.upsample_stage(d, s.t().contiguous().t(), u, 64.0, False)
    with pytest.raises(RuntimeError, match="`sdf` must be"):
        U.upsample_stage(d, s[:, :-1].contiguous(), u, 64.0, False)
    with pytest.raises(RuntimeError, match="`u` must be"):
        U.upsample_stage(d, s, u.expand(3, 9).contiguous(), 64.0, False)
    with pytest.raises(RuntimeError, match="n >= 2"):
        U.upsample_stage(d[:, :1].contiguous(), s[:, :1].contiguous(), u, 64.0, False)
    fine, merged, order = U.upsample_stage(d[:0], s[:0], u, 64.0, False)
    assert fine.shape == (0, 9) and merged.shape == order.shape == (0, 26)
