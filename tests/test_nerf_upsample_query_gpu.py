"""GPU: nerf_ray_query_march_occ_multi_upsample_compressed on the fused route (FUSED_UPSAMPLE_NERF: one launch each of the two packed
stages) against the same driver on the pack-op chain, on the 12 x 12 ray, 32^3 shell scene of tests/test_neus_packed_query_gpu.py with
an analytic density.

Rays, pack shapes and details must be identical.  The depths may differ as two float32 evaluations of the same chain do: by
4 e_ref + one ulp of the largest depth, e_ref = the distance between the float32 and the float64 run of the restatement
(tests/nerf_upsample_ref.py) on the marched depths of this scene, read back from the device once.

Identical packs need compression decisions that rounding cannot flip: the density is so thin (the optical depth along a ray stays
below 3) that no transmittance comes near the early stop of 1e-4, which is asserted on the float64 run; the compression then drops
exactly the samples whose interval is empty."""
import os
import sys

import numpy as np
import pytest
import torch

import nerf_upsample_ref as ref

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
pytestmark = pytest.mark.gpu

NUM_FINE, PEAK, RADIUS, WIDTH = 8, 2.0, 0.62, 0.1


def density(x):
    return PEAK * (1 + 0.48 * x[..., 2]) * torch.exp(-((x.norm(dim=-1) - RADIUS) / WIDTH) ** 2)


class ShellDensity(torch.nn.Module):
    """analytic model: a soft density shell, a position- and view-dependent colour; the protocol of the NeRF drivers"""
    use_view_dirs = True

    def __init__(self, accel):
        super().__init__()
        self.accel = accel
        self.seen = []

    def query_density(self, x, **kw):
        self.seen.append(("query_density", x.shape[0], sorted(kw)))
        return density(x)

    def forward_density(self, x, **kw):
        self.seen.append(("forward_density", x.shape[0], sorted(kw)))
        return dict(sigma=density(x))

    def forward(self, x, v=None, **kw):
        self.seen.append(("forward", x.shape[0], sorted(kw) + ([] if v is None else ["v"])))
        return dict(sigma=density(x), rgb=torch.sigmoid(x + (v if v is not None else 0)))


def _scene(dev, side=12, res=32, empty=False, cls=ShellDensity):
    from demo_field import StaticOccGridAccel, pinhole_rays
    c = (np.stack(np.meshgrid(*[np.arange(res)] * 3, indexing="ij"), -1) + 0.5) / res * 2 - 1
    r = np.linalg.norm(c, axis=-1)
    occ = (r > 0.45) & (r < 0.8) & (not empty)
    model = cls(StaticOccGridAccel(torch.from_numpy(occ).to(dev), 0.03, max_steps=128)).eval()
    o, d, near, far = pinhole_rays(side, dev, fov=0.25)
    n = side * side
    return model, dict(num_rays=n, rays_o=o, rays_d=d, near=near, far=far, rays_inds=torch.arange(n, device=dev))


def _transmittance_margin(o, v, depths, deltas):
    """rows of final samples [K, w] in float64 -> the smallest |T / 1e-4 - 1| over their transmittances"""
    alpha = 1 - torch.exp(-density(o[:, None, :] + v[:, None, :] * depths[..., None]) * deltas)
    T = torch.cat([torch.ones_like(alpha[:, :1]), torch.cumprod(1 - alpha, -1)], -1)
    return (T / 1e-4 - 1).abs().min().item()


_E_REF = {}


def e_ref_of(model, rays, num_coarse, combine):
    """computed once per (num_coarse, combine) and shared: (e_ref, the largest depth, the transmittance margin of the float64 run)"""
    key = (num_coarse, combine)
    if key not in _E_REF:
        from nr3d_lib_amd.graphics.nerf import nerf_ray_query as rq
        with torch.no_grad():
            marched = rq._march(model, rays, rays["rays_o"], rays["rays_d"], rays["near"], rays["far"], False, {})
        hit, pi = marched.ridx_hit.cpu(), marched.pack_infos.cpu()
        assert pi[0, 0] == 0 and torch.equal(pi[1:, 0], (pi[:, 0] + pi[:, 1])[:-1]) and (pi[:, 1] >= 1).all(), "the marcher's packs tile"
        assert 0 < hit.numel() < rays["num_rays"], "rays with and without marched samples"
        o, v = rays["rays_o"].cpu(), rays["rays_d"].cpu()
        t, dt = marched.depth_samples.view(-1).cpu(), marched.deltas.view(-1).cpu()
        R, m = o.shape[0], NUM_FINE + 1
        coarse = ref.coarse_rows(rays["near"].cpu(), rays["far"].cpu(), num_coarse) if num_coarse else None
        out = {}
        for dtype in (torch.float32, torch.float64):
            if num_coarse and combine:
                lens = torch.zeros(R, dtype=torch.int64)
                lens[hit] = pi[:, 1]
                a = ref.merge(coarse, t, torch.stack([torch.cumsum(lens, 0) - lens, lens], -1), o, v, dtype)
                sigma = density(o.to(dtype)[a["ridx_all"]] + v.to(dtype)[a["ridx_all"]] * a["depths_all"][:, None])
                r = ref.stage(a["depths_all"], sigma, a["deltas_all"], a["pack_infos_out"], ref.shared_u(m), coarse=coarse, dtype=dtype)
                rows = torch.arange(R)
            else:
                ridx = torch.repeat_interleave(hit, pi[:, 1])
                sigma = density(o.to(dtype)[ridx] + v.to(dtype)[ridx] * t.to(dtype)[:, None])
                r = ref.stage(t, sigma, dt, pi, ref.shared_u(m), coarse=coarse, coarse_row=hit if num_coarse else None, dtype=dtype)
                rows = hit
            out[dtype] = (r["merged"], r["deltas"], rows)
        d64, dl64, rows = out[torch.float64]
        margin = _transmittance_margin(o.double()[rows], v.double()[rows], d64, dl64)
        if num_coarse:          # the rays that keep their coarse row alone
            margin = min(margin, _transmittance_margin(o.double(), v.double(), coarse.double(),
                                                       torch.cat([coarse.double().diff(dim=-1), torch.zeros(R, 1, dtype=torch.float64)], -1)))
        _E_REF[key] = ((out[torch.float32][0].double() - d64).abs().max().item(), float(d64.abs().max()), margin)
    return _E_REF[key]


@pytest.mark.parametrize("with_rgb", [True, False])
@pytest.mark.parametrize("combine", [True, False])
@pytest.mark.parametrize("num_coarse", [0, 16])
def test_routes_agree(dev, monkeypatch, num_coarse, combine, with_rgb):
    from nr3d_lib_amd.graphics.nerf import nerf_ray_query as rq
    model, rays = _scene(dev)
    kw = dict(with_rgb=with_rgb, num_coarse=num_coarse, num_fine=NUM_FINE, combine_marched_and_coarse=combine)
    e_ref, d_max, margin = e_ref_of(model, rays, num_coarse, combine)
    assert margin > 1e-3, f"a transmittance within {margin:.2e} of the early stop"
    with torch.no_grad():
        monkeypatch.setattr(rq, "FUSED_UPSAMPLE_NERF", True)
        vb_f, det_f = rq.nerf_ray_query_march_occ_multi_upsample_compressed(model, rays, **kw)
        calls_f = list(model.seen)
        model.seen.clear()
        monkeypatch.setattr(rq, "FUSED_UPSAMPLE_NERF", False)
        vb_t, det_t = rq.nerf_ray_query_march_occ_multi_upsample_compressed(model, rays, **kw)
    assert calls_f == model.seen and [c[0] for c in calls_f] == ["query_density", "query_density", "forward" if with_rgb else "forward_density"]
    assert vb_f["type"] == vb_t["type"] == "packed" and set(vb_f) == set(vb_t)
    assert set(vb_t) == {"type", "rays_inds_hit", "pack_infos_hit", "t", "deltas", "sigma", "opacity_alpha"} | ({"rgb"} if with_rgb else set())
    assert torch.equal(vb_f["rays_inds_hit"], vb_t["rays_inds_hit"]) and torch.equal(vb_f["pack_infos_hit"], vb_t["pack_infos_hit"])
    assert set(det_f) == set(det_t) == {"render.num_per_ray0", "march.num_per_ray", "render.num_per_ray"}
    assert all(torch.equal(det_f[k], det_t[k]) for k in det_t)
    assert all(vb_f[k].shape == vb_t[k].shape for k in vb_t if torch.is_tensor(vb_t[k]))
    # with coarse samples every ray has a pack before the compression; the rays that pass the shell by lose theirs in it
    assert det_t["render.num_per_ray0"].numel() == (rays["num_rays"] if num_coarse else det_t["march.num_per_ray"].numel())
    assert vb_t["rays_inds_hit"].numel() == vb_t["pack_infos_hit"].shape[0] == det_t["render.num_per_ray"].numel()
    assert vb_t["t"].numel() == int(vb_t["pack_infos_hit"][:, 1].sum()) and (vb_t["pack_infos_hit"][:, 1] > 0).all()
    diff = (vb_f["t"].double() - vb_t["t"].double()).abs().max().item()
    allowed = 4 * e_ref + float(np.spacing(np.float32(d_max)))
    print(f"num_coarse={num_coarse} combine={combine} with_rgb={with_rgb}: |fused - chain| {diff:.3e}  e_ref {e_ref:.3e}  allowed {allowed:.3e}  "
          f"transmittance margin {margin:.3e}")
    assert diff <= allowed


@pytest.mark.parametrize("num_coarse,combine", [(16, True), (16, False), (0, True)])
def test_one_launch_of_each_stage(dev, monkeypatch, num_coarse, combine):
    from nr3d_lib_amd.bindings import _nerf_upsample as U
    from nr3d_lib_amd.graphics.nerf import nerf_ray_query as rq
    calls, real_a, real_b = [], U.merge_rows_packs, U.upsample_stage_packed
    monkeypatch.setattr(U, "merge_rows_packs", lambda *a, **k: (calls.append("a"), real_a(*a, **k))[1])
    monkeypatch.setattr(U, "upsample_stage_packed", lambda *a, **k: (calls.append("b"), real_b(*a, **k))[1])
    model, rays = _scene(dev)
    kw = dict(num_coarse=num_coarse, num_fine=NUM_FINE, combine_marched_and_coarse=combine)
    monkeypatch.setattr(rq, "FUSED_UPSAMPLE_NERF", True)
    with torch.no_grad():
        rq.nerf_ray_query_march_occ_multi_upsample_compressed(model, rays, **kw)
    assert calls == (["a", "b"] if num_coarse and combine else ["b"])
    calls.clear()
    monkeypatch.setattr(rq, "FUSED_UPSAMPLE_NERF", False)
    with torch.no_grad():
        rq.nerf_ray_query_march_occ_multi_upsample_compressed(model, rays, **kw)
    assert calls == []


def test_a_grid_no_ray_hits_gives_the_coarse_samples(dev, monkeypatch):
    from nr3d_lib_amd.graphics.nerf import nerf_ray_query as rq
    model, rays = _scene(dev, empty=True)
    out = []
    for fused in (True, False):
        monkeypatch.setattr(rq, "FUSED_UPSAMPLE_NERF", fused)
        with torch.no_grad():
            out.append(rq.nerf_ray_query_march_occ_multi_upsample_compressed(model, rays, num_coarse=16, num_fine=NUM_FINE))
            assert rq.nerf_ray_query_march_occ_multi_upsample_compressed(model, rays, num_coarse=0, num_fine=NUM_FINE)[0]["type"] == "empty"
    (vb, det), (vb2, det2) = out
    assert vb["type"] == "packed" and set(det) == {"render.num_per_ray0", "render.num_per_ray"}
    assert (det["render.num_per_ray0"] == 16).all() and det["render.num_per_ray0"].numel() == rays["num_rays"]
    coarse = ref.coarse_rows(rays["near"], rays["far"], 16)
    kept = vb["rays_inds_hit"]
    assert (vb["pack_infos_hit"][:, 1] <= 16).all() and vb["t"].numel() == int(vb["pack_infos_hit"][:, 1].sum())
    ridx = torch.repeat_interleave(kept, vb["pack_infos_hit"][:, 1])
    assert ((vb["t"][:, None] - coarse[ridx]).abs().amin(-1) <= 4 * float(np.spacing(np.float32(6.0)))).all(), "every depth is a coarse one"
    assert all(torch.equal(vb[k], vb2[k]) for k in vb if torch.is_tensor(vb[k])) and all(torch.equal(det[k], det2[k]) for k in det)


def test_bypass_alpha_fn_decides_the_compression(dev, monkeypatch):
    from nr3d_lib_amd.graphics.nerf import nerf_ray_query as rq
    model, rays = _scene(dev)
    # a constant opacity of 0.3: T_i = 0.7^i >= 1e-4 for i <= 25 (0.7^25 = 1.3e-4, 0.7^26 = 9.4e-5), so 26 samples of a pack survive
    bypass = lambda x, **kw: torch.full((x.shape[0],), 0.3, device=x.device)      # noqa: E731
    out = []
    for fused in (True, False):
        monkeypatch.setattr(rq, "FUSED_UPSAMPLE_NERF", fused)
        model.seen.clear()
        with torch.no_grad():
            out.append(rq.nerf_ray_query_march_occ_multi_upsample_compressed(model, rays, num_coarse=16, num_fine=32, bypass_alpha_fn=bypass))
        assert [c[0] for c in model.seen] == ["query_density", "forward"], "the bypass replaces the second density query"
    (vb, det), (vb2, det2) = out
    assert (det["render.num_per_ray0"] == 16 + 33).all() and (det["render.num_per_ray"] == 26).all()
    assert torch.equal(vb["pack_infos_hit"], vb2["pack_infos_hit"]) and torch.equal(vb["rays_inds_hit"], vb2["rays_inds_hit"])
    with pytest.raises(AssertionError, match="at most one"):
        rq.nerf_ray_query_march_occ_multi_upsample_compressed(model, rays, bypass_alpha_fn=bypass, bypass_sigma_fn=bypass)
    with torch.no_grad():
        vb3, _ = rq.nerf_ray_query_march_occ_multi_upsample_compressed(model, rays, num_coarse=16, num_fine=NUM_FINE,
                                                                       bypass_sigma_fn=lambda x, **kw: torch.zeros_like(x[:, 0]))
    assert vb3["type"] == "empty", "no opacity anywhere: nothing is left after the compression"


class PerRayModel(ShellDensity):
    use_ts, use_h_appear, fwd_density_use_pix, use_bidx = True, True, True, True


def test_per_ray_attributes_reach_the_queries(dev, monkeypatch):
    from nr3d_lib_amd.graphics.nerf import nerf_ray_query as rq
    model, rays = _scene(dev, cls=PerRayModel)
    n = rays["num_rays"]
    rays.update(rays_ts=torch.rand(n, device=dev), rays_h_appear=torch.rand(n, 4, device=dev), rays_pix=torch.rand(n, 2, device=dev),
                rays_bidx=torch.arange(n, device=dev) % 3)
    for fused in (True, False):
        monkeypatch.setattr(rq, "FUSED_UPSAMPLE_NERF", fused)
        model.seen.clear()
        with torch.no_grad():
            vb, _ = rq.nerf_ray_query_march_occ_multi_upsample_compressed(model, rays, num_coarse=16, num_fine=NUM_FINE)
        assert [c[2] for c in model.seen] == [["bidx", "pix", "ts"], ["bidx", "pix", "ts"], ["bidx", "h_appear", "pix", "ts", "v"]]
        assert torch.equal(vb["rays_bidx_hit"], rays["rays_bidx"][vb["rays_inds_hit"]])
