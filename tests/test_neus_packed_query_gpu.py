"""GPU: the march-occ NeuS drivers with their up-sampling on the fused route (FUSED_UPSAMPLE_PACKED: one launch of the packed stage
per factor) against the same drivers on the pack-op chain, on the 12 x 12 ray, 32^3 shell scene of tests/test_neus_query_gpu.py.

Rays, pack shapes and details must be identical.  The depths may differ as two float32 evaluations of the same chain do: by
4 e_ref + one ulp of the largest depth, e_ref = the distance between the float32 and the float64 run of the loop restatement
(tests/neus_packed_ref.py) on the marched depths of this scene, read back from the device."""
import os
import sys

import numpy as np
import pytest
import torch

import neus_packed_ref as ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
pytestmark = pytest.mark.gpu


class SphereSDF(torch.nn.Module):
    """analytic model: sdf = |x| - r; colour = position-dependent; the protocol of the NeuS driver"""
    use_view_dirs = True

    def __init__(self, accel, radius=0.62, inv_s=48.0):
        super().__init__()
        self.accel, self.radius, self.inv_s = accel, radius, inv_s

    def forward_inv_s(self):
        return self.inv_s

    def forward_sdf(self, x, **kw):
        return dict(sdf=x.norm(dim=-1) - self.radius)

    def forward(self, x, v=None, nablas_has_grad=False, with_rgb=True, with_normal=True, **kw):
        out = dict(sdf=x.norm(dim=-1) - self.radius)
        if with_normal:
            out["nablas"] = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-10)
        if with_rgb:
            out["rgb"] = torch.sigmoid(x + (v if v is not None else 0))
        return out


def _scene(dev, side=12, res=32):
    from demo_field import StaticOccGridAccel, pinhole_rays
    c = (np.stack(np.meshgrid(*[np.arange(res)] * 3, indexing="ij"), -1) + 0.5) / res * 2 - 1
    r = np.linalg.norm(c, axis=-1)
    occ = (r > 0.45) & (r < 0.8)
    model = SphereSDF(StaticOccGridAccel(torch.from_numpy(occ).to(dev), 0.03, max_steps=128)).eval()
    o, d, near, far = pinhole_rays(side, dev, fov=0.25)
    n = side * side
    return model, dict(num_rays=n, rays_o=o, rays_d=d, near=near, far=far, rays_inds=torch.arange(n, device=dev))


_E_REF = {}


def e_ref_of(model, rays, factors, est, num_fine):
    """computed once per (factors, formula) and shared: (e_ref, the largest marched depth)"""
    key = (tuple(factors), est, num_fine)
    if key not in _E_REF:
        from nr3d_lib_amd.graphics.neus import neus_ray_query as rq
        with torch.no_grad():
            marched = rq._march(model, rays, rays["rays_o"], rays["rays_d"], rays["near"], rays["far"], False, {})
        hit, pi = marched.ridx_hit, marched.pack_infos.cpu()
        assert pi[0, 0] == 0 and torch.equal(pi[1:, 0], (pi[:, 0] + pi[:, 1])[:-1]) and (pi[:, 1] >= 1).all(), "the marcher's packs tile"
        args = (rays["rays_o"][hit], rays["rays_d"][hit], marched.depth_samples, pi, num_fine, factors, 64.0, est)
        d32 = ref.upsample_loop(*args, dtype=torch.float32, radius=model.radius)
        d64 = ref.upsample_loop(*args, dtype=torch.float64, radius=model.radius)
        _E_REF[key] = ((d32.double() - d64).abs().max().item(), marched.depth_samples.abs().max().item())
    return _E_REF[key]


@pytest.mark.parametrize("est", [False, True])
@pytest.mark.parametrize("factors", [[1, 4, 16], [1]])
@pytest.mark.parametrize("num_coarse", [0, 16])
@pytest.mark.parametrize("compressed", [False, True])
def test_drivers_agree_on_both_routes(dev, monkeypatch, compressed, num_coarse, factors, est):
    from nr3d_lib_amd.graphics.neus import neus_ray_query as rq
    driver = rq.neus_ray_query_march_occ_multi_upsample_compressed if compressed else rq.neus_ray_query_march_occ_multi_upsample
    model, rays = _scene(dev)
    kw = dict(num_coarse=num_coarse, num_fine=8, upsample_inv_s_factors=factors, upsample_use_estimate_alpha=est)
    with torch.no_grad():
        monkeypatch.setattr(rq, "FUSED_UPSAMPLE_PACKED", True)
        vb_f, det_f = driver(model, rays, **kw)
        monkeypatch.setattr(rq, "FUSED_UPSAMPLE_PACKED", False)
        vb_t, det_t = driver(model, rays, **kw)
    e_ref, d_max = e_ref_of(model, rays, factors, est, 8)
    assert vb_f["type"] == vb_t["type"] != "empty" and set(vb_f) == set(vb_t)
    assert torch.equal(vb_f["rays_inds_hit"], vb_t["rays_inds_hit"])
    for k in ("pack_infos_hit", "num_per_hit"):
        if k in vb_t:
            assert torch.equal(torch.as_tensor(vb_f[k]), torch.as_tensor(vb_t[k])), k
    assert set(det_f) == set(det_t) and all(torch.equal(torch.as_tensor(det_f[k]), torch.as_tensor(det_t[k])) for k in det_t)
    assert vb_f["t"].shape == vb_t["t"].shape and vb_f["rgb"].shape == vb_t["rgb"].shape
    diff = (vb_f["t"].double() - vb_t["t"].double()).abs().max().item()
    allowed = 4 * e_ref + float(np.spacing(np.float32(d_max)))
    print(f"compressed={compressed} num_coarse={num_coarse} factors={factors} est={est}: |fused - torch| {diff:.3e}  e_ref {e_ref:.3e}  "
          f"allowed {allowed:.3e}")
    assert diff <= allowed


@pytest.mark.parametrize("factors", [[1, 4, 16], [1]])
def test_one_stage_launch_per_factor(dev, monkeypatch, factors):
    from nr3d_lib_amd.bindings import _neus_upsample as U
    from nr3d_lib_amd.graphics.neus import neus_ray_query as rq
    calls, real = [], U.upsample_stage_packed

    def counted(*a, merge=True, need_sdf=True):
        calls.append((merge, need_sdf))
        return real(*a, merge=merge, need_sdf=need_sdf)

    monkeypatch.setattr(U, "upsample_stage_packed", counted)
    monkeypatch.setattr(rq, "FUSED_UPSAMPLE_PACKED", True)
    model, rays = _scene(dev)
    for driver in (rq.neus_ray_query_march_occ_multi_upsample, rq.neus_ray_query_march_occ_multi_upsample_compressed):
        calls.clear()
        with torch.no_grad():
            driver(model, rays, num_fine=8, upsample_inv_s_factors=factors)
        assert calls == [(True, True)] * (len(factors) - 1) + [(False, False)]
    calls.clear()
    monkeypatch.setattr(rq, "FUSED_UPSAMPLE_PACKED", False)
    with torch.no_grad():
        rq.neus_ray_query_march_occ_multi_upsample(model, rays, num_fine=8, upsample_inv_s_factors=factors)
    assert calls == []


def test_perturbed_depths_sorted_inside_the_marched_span(dev, monkeypatch):
    from nr3d_lib_amd.bindings import _neus_upsample as U
    from nr3d_lib_amd.graphics.neus import neus_ray_query as rq
    seen, real = [], U.upsample_stage_packed

    def recorded(depth, sdf, pack_infos, u, *a, **kw):
        out = real(depth, sdf, pack_infos, u, *a, **kw)
        seen.append((depth, pack_infos, u, out[0]))
        return out

    monkeypatch.setattr(U, "upsample_stage_packed", recorded)
    monkeypatch.setattr(rq, "FUSED_UPSAMPLE_PACKED", True)
    model, rays = _scene(dev)
    torch.manual_seed(5)
    with torch.no_grad():
        vb, _ = rq.neus_ray_query_march_occ_multi_upsample(model, rays, perturb=True, num_fine=8, upsample_inv_s_factors=[1, 4, 16])
    assert len(seen) == 3 and all(u.shape == (vb["t"].shape[0], 9) for _, _, u, _ in seen), "one stratified row of u per pack"
    depth, pi = seen[0][0], seen[0][1]
    lo, hi = depth[pi[:, 0]], depth[pi[:, 0] + pi[:, 1] - 1]
    for _, _, _, fine in seen:
        assert (fine.diff(dim=-1) >= 0).all() and (fine >= lo[:, None]).all() and (fine <= hi[:, None]).all()
    assert vb["type"] == "batched" and (vb["t"].diff(dim=-1) >= 0).all()
    assert (vb["t"] >= lo[:, None]).all() and (vb["t"] <= hi[:, None]).all()
