"""GPU: the dynamic renderer mixins on the dynamic accelerators, end to end.  An analytic model -- a ball of density (NeRF) or a sphere
SDF (NeuS) whose centre moves along x with the timestamp -- is driven through ``NerfRendererMixinDynamic.ray_query`` ('march_occ') and
``NeusRendererMixinDynamic.ray_query`` ('march_occ_multi_upsample_compressed') on ``OccGridAccelDynamic`` /
``OccGridAccelStaticAndDynamic`` with T = 4 keyframes, 16^3 cells and 256 rays.

The fused and the chain route of the march (``FUSED_DYNAMIC_MARCH``) must give identical volume buffers: integers equal, floats bit for
bit -- the two marches agree in every bit, and everything behind them is the same deterministic code on the same inputs."""
import numpy as np
import pytest
import torch

import dynamic_march_ref as ref

pytestmark = pytest.mark.gpu

KEYS = [-1.0, -1.0 / 3, 1.0 / 3, 1.0]
RES, RADIUS, PEAK = 16, 0.15, 40.0
MARCH = dict(step_size=0.02, max_steps=128)


def centre(ts):
    """the ball of timestamp ts: 0.6 * ts along x -- the keyframes' balls are 0.4 apart, more than a diameter"""
    return torch.stack([0.6 * ts, torch.zeros_like(ts), torch.zeros_like(ts)], -1)


def density(x, ts):
    return PEAK * ((RADIUS - (x - centre(ts)).norm(dim=-1)) / 0.03).clamp(0, 1)          # compact support: exactly 0 outside the ball


STATIC_C = (0.0, 0.6, 0.0)


def density_static(x):
    return PEAK * ((RADIUS - (x - x.new_tensor(STATIC_C)).norm(dim=-1)) / 0.03).clamp(0, 1)


class MovingBall(torch.nn.Module):
    """the protocol of the NeRF drivers, every query with `ts`; `static` adds a ball that does not move"""

    def __init__(self, static=False, device=None):
        super().__init__()
        from nr3d_lib_amd.models.spatial import AABBDynamicSpace
        self.space = AABBDynamicSpace(device=device)
        self.static = static

    def query_density_static(self, x):
        return density_static(x)

    def query_density_dynamic(self, x, ts):
        return density(x, ts)

    def query_density(self, x, ts):
        return density(x, ts) + (density_static(x) if self.static else 0)

    def forward_density(self, x, ts):
        return dict(sigma=self.query_density(x, ts))

    def forward(self, x, ts):
        out = dict(sigma=self.query_density(x, ts), rgb=torch.sigmoid(3 * x))
        if self.static:
            out.update(sigma_static=density_static(x), sigma_dynamic=density(x, ts), rgb_static=torch.sigmoid(3 * x),
                       rgb_dynamic=torch.sigmoid(-3 * x), flow_fwd=x * ts.unsqueeze(-1), flow_bwd=-x)
        return out


def _voxel_centres(dev):
    c = (torch.arange(RES, device=dev) + 0.5) / RES * 2 - 1
    return torch.stack(torch.meshgrid(c, c, c, indexing="ij"), -1)


def _analytic_occupancy(dev, c):
    """voxels whose centre is within the ball's radius plus half a voxel diagonal of c"""
    return (_voxel_centres(dev) - torch.as_tensor(c, device=dev, dtype=torch.float32)).norm(dim=-1) < RADIUS + 3 ** 0.5 / RES


def _nerf_model(dev, static):
    from nr3d_lib_amd.models.accelerations.occgrid_accel import OccGridAccelDynamic, OccGridAccelStaticAndDynamic
    from nr3d_lib_amd.models.fields_dynamic.nerf import NerfRendererMixinDynamic

    class Model(NerfRendererMixinDynamic, MovingBall):
        pass

    model = Model(static=static, device=dev)
    common = dict(resolution=RES, device=dev, occ_val_fn_cfg=dict(type="density"), occ_thre=0.01,
                  init_cfg=dict(mode="from_net", num_steps=4, num_pts=2 ** 17), update_from_net_cfg=dict(num_steps=1, num_pts=2 ** 12))
    if static:
        model.accel = OccGridAccelStaticAndDynamic(model.space, KEYS, occ_static_cfg={}, occ_dynamic_cfg={}, **common)
    else:
        model.accel = OccGridAccelDynamic(model.space, KEYS, **common)
    torch.manual_seed(0)
    model.training_initialize()
    return model.eval()


def _rays(dev, ts_of_group, aim_of_group):
    """256 rays in 4 groups of 64, nearly along +z from z = -3, group g through the ball of keyframe aim_of_group[g] (a disc of
    radius 0.08 around its centre), carrying the timestamp KEYS[ts_of_group[g]]"""
    rng = np.random.default_rng(3)
    o, d, ts = [], [], []
    for g in range(4):
        r, phi = 0.08 * np.sqrt(rng.random(64)), rng.uniform(0, 2 * np.pi, 64)
        cx = 0.6 * KEYS[aim_of_group[g]]
        o.append(np.stack([cx + r * np.cos(phi), r * np.sin(phi), np.full(64, -3.0)], 1))
        dd = np.stack([rng.normal(0, 2e-3, 64), rng.normal(0, 2e-3, 64), np.ones(64)], 1)
        d.append(dd / np.linalg.norm(dd, axis=1, keepdims=True))
        ts.append(np.full(64, KEYS[ts_of_group[g]]))
    f = lambda a: torch.from_numpy(np.concatenate(a).astype(np.float32)).to(dev)     # noqa: E731
    return dict(rays_o=f(o), rays_d=f(d), rays_ts=f(ts))


def _mixed_ts(dev):
    """128 timestamps of every finite kind: the lookup tables' values (on, between, below and above keys) and the exact midpoints of
    this test's keyframes (ties).  The model is evaluated AT the ray's timestamp, so the non-finite ones stay in the march tests."""
    v = np.concatenate([ref.TABLE_T, ref.TABLE2_T, [-2.0 / 3, 0.0, 2.0 / 3]]).astype(np.float32)
    return torch.from_numpy(np.resize(v[np.isfinite(v)], 128)).to(dev)


CFG = dict(query_mode="march_occ", with_rgb=True, with_normal=False, perturb=False, query_param=dict(march_cfg=MARCH))


def _both_routes(monkeypatch, fn):
    import nr3d_lib_amd.graphics.raymarch.occgrid_raymarch as m
    out = []
    for fused in (True, False):
        monkeypatch.setattr(m, "FUSED_DYNAMIC_MARCH", fused)
        out.append(fn())
    return out


def _assert_same_buffers(a, b):
    assert a["type"] == b["type"] != "empty" and sorted(a) == sorted(b)
    n = 0
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            x, y = a[k].detach().cpu().numpy(), b[k].detach().cpu().numpy()
            if x.dtype.kind == "f":
                x, y = x.view(np.int32), y.view(np.int32)
            assert np.array_equal(x, y), f"{k}: {int((x != y).sum())} of {x.size} entries differ between the routes"
            n += 1
        else:
            assert a[k] == b[k], k
    return n


@pytest.mark.parametrize("static", [False, True], ids=["OccGridAccelDynamic", "OccGridAccelStaticAndDynamic"])
def test_nerf_march_occ_routes_identical_and_frames_separate(dev, monkeypatch, static):
    model = _nerf_model(dev, static)
    grid = model.accel.occ_dynamic.occ_grid if static else model.accel.get_occ_grid()
    # init from the network: slice k holds the ball of keyframe k and nothing of the others
    for k, key in enumerate(KEYS):
        near_k = _analytic_occupancy(dev, (0.6 * key, 0.0, 0.0))
        assert int(grid[k].sum()) >= 8 and not bool((grid[k] & ~near_k).any()), f"slice {k}"
    if static:
        sta = model.accel.occ_static.occ_grid
        assert int(sta.sum()) >= 8 and not bool((sta & ~_analytic_occupancy(dev, STATIC_C)).any())
        assert torch.equal(model.accel.get_occ_grid(), grid | sta)

    # (1) timestamps of every finite kind on every other ray: both routes, same buffers
    rays = _rays(dev, [0, 1, 2, 3], [0, 1, 2, 3])
    rays["rays_ts"][::2] = _mixed_ts(dev)
    cfg = dict(CFG, with_static_dynamic=static, with_flow=static)

    def run():
        return model.ray_query(ray_input=rays, config=cfg, return_buffer=True, return_details=True, render_per_obj_individual=True)
    fused, chain = _both_routes(monkeypatch, run)
    assert _assert_same_buffers(fused["volume_buffer"], chain["volume_buffer"]) >= 6
    for k in fused["rendered"]:
        assert torch.equal(fused["rendered"][k], chain["rendered"][k]), k
    assert torch.equal(fused["details"]["march.num_per_ray"], chain["details"]["march.num_per_ray"])
    if static:
        assert {"opacity_alpha_static", "opacity_alpha_dynamic", "flow_fwd"} <= set(fused["volume_buffer"])
        assert {"mask_static", "mask_dynamic", "depth_static", "rgb_dynamic", "flow_fwd", "flow_bwd"} <= set(fused["rendered"])

    # (2) a ray with the timestamp of keyframe k sees the ball of keyframe k ...
    monkeypatch.setattr(__import__("nr3d_lib_amd.graphics.raymarch.occgrid_raymarch", fromlist=["x"]), "FUSED_DYNAMIC_MARCH", True)
    seen = model.ray_query(ray_input=_rays(dev, [0, 1, 2, 3], [0, 1, 2, 3]), config=cfg, render_per_obj_individual=True)["rendered"]
    assert float(seen["mask_volume"].min()) > 0.9, "every ray through the ball of its own keyframe is opaque"
    assert float((seen["depth_volume"] - 3.0).abs().max()) < RADIUS + 0.05
    # ... and not the ball of keyframe k + 1 or k - 1: aimed at a neighbour's ball, it meets no density at all
    for shift in (1, -1):
        aim = [(g + shift) % 4 for g in range(4)]
        other = model.ray_query(ray_input=_rays(dev, [0, 1, 2, 3], aim), config=cfg, render_per_obj_individual=True)["rendered"]
        assert float(other["mask_volume"].abs().max()) == 0.0, f"shift {shift}"
    if static:
        assert float(seen["mask_static"].abs().max()) == 0.0 and float(seen["mask_dynamic"].min()) > 0.9


@pytest.mark.parametrize("static", [False, True], ids=["OccGridAccelDynamic", "OccGridAccelStaticAndDynamic"])
def test_collect_samples_then_step_touches_one_slice(dev, static):
    from nr3d_lib_amd.models.accelerations.occgrid_accel import OccGridAccelDynamic, OccGridAccelStaticAndDynamic
    from nr3d_lib_amd.models.spatial import AABBDynamicSpace
    space = AABBDynamicSpace(device=dev)
    common = dict(resolution=RES, device=dev, occ_val_fn_cfg=dict(type="density"), init_cfg=dict(mode="constant", constant_value=0.0),
                  update_from_net_cfg=dict(num_steps=1, num_pts=2 ** 12), n_steps_between_update=16)
    zero = lambda x, ts=None: torch.zeros(x.shape[:-1], device=dev)        # noqa: E731
    pts = torch.tensor([[0.03, 0.03, 0.03], [0.55, -0.55, 0.2], [0.57, -0.57, 0.21]], device=dev)     # voxels (8, 8, 8) and (12, 3, 9)
    ts = torch.tensor([0.3, 0.4, 0.34], device=dev)                         # all nearest to KEYS[2] = 1/3
    val = torch.tensor([5.0, 7.0, 3.0], device=dev)
    if static:
        acc = OccGridAccelStaticAndDynamic(space, KEYS, occ_static_cfg={}, occ_dynamic_cfg={}, **common).train()
        acc.init(zero, zero)
        acc.collect_samples(pts, ts, val_static=val * 2, val_dynamic=val)
        acc.step(16, zero, zero)
        stack, single = acc.occ_dynamic, acc.occ_static
    else:
        acc = OccGridAccelDynamic(space, KEYS, **common).train()
        acc.init(zero)
        acc.collect_samples(pts, ts, val)
        acc.step(16, zero)
        stack, single = acc.occ, None
    want = torch.zeros(RES, RES, RES, device=dev)
    want[8, 8, 8], want[12, 3, 9] = 5.0, 7.0
    for k in range(4):
        assert torch.equal(stack.occ_val_grid[k], want if k == 2 else torch.zeros_like(want)), f"slice {k}"
        assert torch.equal(stack.occ_grid[k], (want > 0) if k == 2 else torch.zeros_like(want, dtype=torch.bool)), f"slice {k}"
    if single is not None:
        assert torch.equal(single.occ_val_grid, want * 2) and int(single.occ_grid.sum()) == 2
    # evaluation mode: samples are not collected
    acc.eval()
    acc.collect_samples(pts, ts.new_full((3,), -1.0), *((val, val) if static else (val,)))
    acc.train()
    acc.step(32, *((zero, zero) if static else (zero,)))
    assert float(stack.occ_val_grid[0].abs().max()) == 0.0


# ---- NeuS ------------------------------------------------------------------------------------------------------------------------
class MovingSphereSDF(torch.nn.Module):
    """the protocol of the NeuS drivers, every query with `ts`"""

    def __init__(self, device=None):
        super().__init__()
        from nr3d_lib_amd.models.spatial import AABBDynamicSpace
        self.space = AABBDynamicSpace(device=device)
        self.seen_ts = []

    def _sdf(self, x, ts):
        return (x - centre(ts)).norm(dim=-1) - RADIUS

    def forward_inv_s(self):
        return 64.0

    def query_sdf(self, x, ts):
        return self._sdf(x, ts)

    def forward_sdf(self, x, ts):
        self.seen_ts.append(ts)
        return dict(sdf=self._sdf(x, ts))

    def forward_sdf_nablas(self, x, ts):
        diff = x - centre(ts)
        return dict(sdf=self._sdf(x, ts), nablas=diff / diff.norm(dim=-1, keepdim=True).clamp_min(1e-10))

    def forward(self, x, ts, nablas_has_grad=False, with_rgb=True, with_normal=True):
        out = self.forward_sdf_nablas(x, ts)
        if with_rgb:
            out["rgb"] = torch.sigmoid(3 * x)
        return out


def test_neus_march_occ_multi_upsample_compressed(dev, monkeypatch):
    from nr3d_lib_amd.models.accelerations.occgrid_accel import OccGridAccelDynamic
    from nr3d_lib_amd.models.fields_dynamic.neus import NeusRendererMixinDynamic

    class Model(NeusRendererMixinDynamic, MovingSphereSDF):
        pass

    model = Model(device=dev)
    model.accel = OccGridAccelDynamic(model.space, KEYS, resolution=RES, device=dev, init_cfg=dict(mode="constant", constant_value=0.0))
    model.accel.init(None)
    for k, key in enumerate(KEYS):
        model.accel.occ.occ_grid[k] = _analytic_occupancy(dev, (0.6 * key, 0.0, 0.0))
    model.eval()
    cfg = dict(query_mode="march_occ_multi_upsample_compressed", with_rgb=True, with_normal=True, perturb=False,
               query_param=dict(march_cfg=MARCH, num_fine=4, upsample_inv_s_factors=[1, 4]))
    rays = _rays(dev, [0, 1, 2, 3], [0, 1, 2, 3])
    rays["rays_ts"][::2] = _mixed_ts(dev)

    def run():
        return model.ray_query(ray_input=rays, config=cfg, return_buffer=True, return_details=True, render_per_obj_individual=True)
    fused, chain = _both_routes(monkeypatch, run)
    assert fused["volume_buffer"]["type"] == "packed"
    assert _assert_same_buffers(fused["volume_buffer"], chain["volume_buffer"]) >= 6
    for k in fused["rendered"]:
        assert torch.equal(fused["rendered"][k], chain["rendered"][k]), k
    assert model.seen_ts and all(t.dtype == torch.float32 for t in model.seen_ts)       # the SDF queries got the rays' timestamps

    seen = model.ray_query(ray_input=_rays(dev, [0, 1, 2, 3], [0, 1, 2, 3]), config=cfg, render_per_obj_individual=True)["rendered"]
    # num_coarse = 0: the buffer holds the fine samples only, and they crowd around the surface crossing.  Along a falling SDF the NeuS
    # opacities telescope to 1 - Phi(s sdf_deepest) / Phi(s sdf_first), which reaches 1 only as far as the samples go into the ball: the
    # ray is held to "more opaque than not" (0.79 - 0.82 on this scene).  The weight sits within |sdf| < 3 / s = 0.047 of the surface,
    # whose depth along these rays (offset <= 0.08 from the axis) is 3 - sqrt(RADIUS^2 - r^2) in [2.85, 2.873]: depth within 0.07 of
    # 2.85, and the unit normals there have n_z <= -sqrt(1 - (0.08 / (RADIUS - 0.047))^2) = -0.63.
    assert float(seen["mask_volume"].min()) > 0.5
    assert float((seen["depth_volume"] - (3.0 - RADIUS)).abs().max()) < 0.07            # the surface, not the centre
    assert float((seen["normals_volume"][:, 2] / seen["mask_volume"]).max()) < -0.6     # facing the camera
    for shift in (1, -1):
        aim = [(g + shift) % 4 for g in range(4)]
        other = model.ray_query(ray_input=_rays(dev, [0, 1, 2, 3], aim), config=cfg, render_per_obj_individual=True)["rendered"]
        assert float(other["mask_volume"].max()) < 1e-3, f"shift {shift}"
    for mode in ("march_occ", "march_occ_multi_upsample_compressed_strategy"):
        with pytest.raises(NotImplementedError):
            model.ray_query(ray_input=rays, config=dict(cfg, query_mode=mode))
    with pytest.raises(RuntimeError, match="Invalid query_mode"):
        model.ray_query(ray_input=rays, config=dict(cfg, query_mode="nope"))
