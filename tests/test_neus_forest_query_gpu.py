"""GPU: the three forest NeuS drivers (graphics.neus.neus_forest_ray_query) and NeuSRendererMixinForest on a 7-block "plus" forest
(level 2, block size 1) around an analytic sphere of radius 0.8 at the hub's centre, so the surface lies in the arm blocks.
OccGridAccelForest learns its grids from that field as tests/test_forest_gpu.py::test_forest_accel_end_to_end does; 12 x 12 rays.

Fused route (FUSED_UPSAMPLE_FOREST: one launch of the block-carrying stage per factor) against the pack-op chain: rays, pack shapes
and details identical; depths within 4 e_ref + one ulp of the largest depth, e_ref = the distance between the float32 and the
float64 run of the loop restatement (tests/neus_forest_ref.py) on the samples the loop starts from (the rule of
tests/test_neus_packed_query_gpu.py); the block indices handed to the last forward_sdf equal except where the restatement proves
a tie -- a new depth whose u lies within tau of a float64 CDF knot, or one that took its label from such a sample; tau is taken
per stage, 4 x |cdf32 - cdf64| of the restatement on that stage's own inputs, and at most 0.5 % of the cases may be ties.  The
march-occ pair is compared on all 144 rays, the coarse driver on those that pass through the sphere (rays_through_the_sphere)."""
import numpy as np
import pytest
import torch

import neus_forest_ref as fref

pytestmark = pytest.mark.gpu

PLUS7 = [(1, 1, 1), (0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2)]
CENTRE = (-0.5, -0.5, -0.5)
SIDE = 12


class ForestSphere(torch.nn.Module):
    """analytic model with the forest drivers' protocol: sdf = |x - c| - r in world space; records the block_inds it is given"""
    use_view_dirs = True

    def __init__(self, space, accel, radius=0.8, inv_s=48.0):
        super().__init__()
        self.space, self.accel, self.inv_s = space, accel, inv_s
        self.radius = torch.nn.Parameter(torch.tensor(radius, device=space.device))
        self.register_buffer("centre", torch.tensor(CENTRE, device=space.device))
        self.sdf_block_inds, self.fwd_block_inds = [], []

    def forward_inv_s(self):
        return self.inv_s

    def forward_sdf(self, x, block_inds=None, **kw):
        assert block_inds is not None and block_inds.shape == x.shape[:-1] and block_inds.dtype == torch.int64
        self.sdf_block_inds.append(block_inds)
        return dict(sdf=(x - self.centre).norm(dim=-1) - self.radius)

    def forward(self, x, v=None, block_inds=None, h_appear=None, nablas_has_grad=False, with_rgb=True, with_normal=True):
        self.fwd_block_inds.append(block_inds)
        out = dict(sdf=(x - self.centre).norm(dim=-1) - self.radius)
        if with_normal:
            out["nablas"] = (x - self.centre) / (x - self.centre).norm(dim=-1, keepdim=True).clamp_min(1e-10)
        if with_rgb:
            out["rgb"] = torch.sigmoid(x + (v if v is not None else 0))
        return out


_SCENE = {}


def scene(dev):
    """built once: (model, ray_input, ray_tested)"""
    if "s" not in _SCENE:
        from nr3d_lib_amd.models.accelerations.occgrid_accel import OccGridAccelForest
        from nr3d_lib_amd.models.spatial import ForestBlockSpace
        torch.manual_seed(0)
        space = ForestBlockSpace(device=dev)
        space.populate(mode="from_corners", corners=PLUS7, level=2, world_origin=[-2., -2, -2], world_block_size=1.0)
        assert space.n_trees == 7
        accel = OccGridAccelForest(space, vox_size=1 / 16, occ_thre=0.3, ema_decay=0.9, n_steps_between_update=2, n_steps_warmup=4,
                                   init_cfg=dict(mode="from_net", num_steps=2, num_pts_per_batch=2 ** 14),
                                   update_from_net_cfg=dict(num_steps=1, num_pts_per_batch=2 ** 13))
        accel.populate()
        centre = torch.tensor(CENTRE, device=dev)

        def query(block_x, bidx):                                    # a shell of radius 0.8 around the hub's centre
            return torch.exp(-(((space.unnormalize_coords(block_x, bidx) - centre).norm(dim=-1) - 0.8) / 0.1) ** 2)
        accel.train()
        assert accel.init(query)
        for it in range(1, 7):
            accel.step(it, query)
        accel.eval()
        a = torch.linspace(-0.45, 0.45, SIDE, device=dev)      # a third of the rays meet the sphere, the corner rays miss every block
        d = torch.stack([torch.ones(SIDE, SIDE, device=dev), *torch.meshgrid(a, a, indexing="ij")], -1).reshape(-1, 3)
        d = torch.nn.functional.normalize(d, dim=-1)
        o = torch.tensor([-3.5, -0.5, -0.5], device=dev).expand_as(d).contiguous()
        ray_input = dict(rays_o=o, rays_d=d, near=0.05, far=8.0)
        model = ForestSphere(space, accel).eval()
        _SCENE["s"] = (model, ray_input, space.ray_test(**ray_input))
        closest = ((centre - o) - ((centre - o) * d).sum(-1, keepdim=True) * d).norm(dim=-1)
        _SCENE["through"] = space.ray_test(o[closest < 0.75].contiguous(), d[closest < 0.75].contiguous(), near=0.05, far=8.0)
    return _SCENE["s"]


def rays_through_the_sphere(dev):
    """ray_test of the rays that pass the centre within 0.75.  The coarse driver steps along EVERY tested ray, and a ray that passes
    the sphere at a distance carries a mass of 1e-6 or less, divided by max(mass, 1e-5): its CDF is rounding noise over a floor, and
    which bin a u falls in is decided by the last bit of sigmoids next to 1.  Labels can be compared where the CDF is a CDF
    (neus_packed_ref.check_preconditions asks the same of its packs); the marched packs lie around the surface and all have mass."""
    scene(dev)
    return _SCENE["through"]


def drivers():
    from nr3d_lib_amd.graphics.neus import neus_forest_ray_query as fq
    return fq, dict(coarse=fq.neus_forest_ray_query_coarse_multi_upsample, march=fq.neus_forest_ray_query_march_occ_multi_upsample,
                    compressed=fq.neus_forest_ray_query_march_occ_multi_upsample_compressed)


def driver_kwargs(name, factors, est, coarse_cfg):
    if name == "coarse":
        return dict(coarse_step_cfg=coarse_cfg or COARSE_DEFAULT, upsample_mode='multistep_estimate', num_fine=8, upsample_inv_s_factors=factors,
                    upsample_use_estimate_alpha=est)
    return dict(coarse_step_cfg=coarse_cfg, march_cfg=MARCH_CFG, num_fine=8, upsample_inv_s_factors=factors,
                upsample_use_estimate_alpha=est)


# Steps of a few hundredths: packs of some ten to thirty samples.  The labels are compared away from CDF knots, and a pack of hundreds of
# samples a thousandth apart has a knot within rounding of most u (the slope estimate divides SDF differences of 1e-3 by the step)
COARSE_CFG = dict(step_mode='depth', max_steps=32, min_step_size=0.05, dt_gamma=0.02)
COARSE_DEFAULT = dict(step_mode='depth', max_steps=64, min_step_size=0.04, dt_gamma=0.0)      # the coarse driver without `with_coarse`
MARCH_CFG = dict(step_size=0.03, max_steps=128)


def loop_input(model, rt, name, coarse_cfg):
    """the samples the up-sampling loop starts from -> (rays_o, rays_d of the packs, depth, blidx, pack_infos)"""
    seg = [rt[k] for k in ('seg_block_inds', 'seg_entries', 'seg_exits', 'seg_pack_infos')]
    with torch.no_grad():
        if name == "coarse":
            r = model.space.ray_step_coarse(rt['rays_o'], rt['rays_d'], rt['near'], rt['far'], *seg, **(coarse_cfg or COARSE_DEFAULT))
            hit, depth, blidx, pi = r['ridx_hit'], r['depth_samples'], r['blidx'], r['pack_infos']
        else:
            r = model.accel.ray_march(rt['rays_o'], rt['rays_d'], rt['near'], rt['far'], *seg, **MARCH_CFG)
            hit, depth, blidx, pi = r.ridx_hit, r.depth_samples, r.blidx, r.pack_infos
    return rt['rays_o'][hit], rt['rays_d'][hit], depth, blidx, pi


_REF = {}


def restated(model, rt, name, coarse_cfg, factors, est):
    """computed once per configuration and shared: (e_ref, largest depth, excused bool [P, S m] of the float64 run, its labels, tau,
    excused for every sample of the union behind the last stage)"""
    key = (name if name == "coarse" else "march", bool(coarse_cfg) if name == "coarse" else False, tuple(factors), est)
    if key not in _REF:
        o, v, depth, blidx, pi = (t.cpu() for t in loop_input(model, rt, name, coarse_cfg))
        assert pi[0, 0] == 0 and torch.equal(pi[1:, 0], (pi[:, 0] + pi[:, 1])[:-1]) and (pi[:, 1] >= 1).all(), "the packs tile"
        centre, radius = torch.tensor(CENTRE), float(model.radius.detach())
        u = torch.linspace(0., 1., 9 + 2)[1:-1]                                  # cdf_positions, unperturbed
        args = (o, v, depth, blidx, pi, 8, factors, 64.0, est, u)
        r32 = fref.upsample_loop(lambda x: (x - centre.to(x.dtype)).norm(dim=-1) - radius, *args, dtype=torch.float32)
        r64 = fref.upsample_loop(lambda x: (x - centre.to(x.dtype)).norm(dim=-1) - radius, *args, dtype=torch.float64, ties=True)
        tau = max(r64['taus'])                                                   # one per stage, on the stage's own inputs
        _REF[key] = ((r32['fine'].double() - r64['fine']).abs().max().item(), depth.abs().max().item(), r64['excused'], r64['blidx'], tau,
                     r64['excused_union'])
    return _REF[key]


@pytest.mark.parametrize("est", [False, True])
@pytest.mark.parametrize("factors", [[1, 4, 16], [1]])
@pytest.mark.parametrize("with_coarse", [False, True])
@pytest.mark.parametrize("name", ["coarse", "march", "compressed"])
def test_drivers_agree_on_both_routes(dev, monkeypatch, name, with_coarse, factors, est):
    model, _, rt = scene(dev)
    if name == "coarse":
        rt = rays_through_the_sphere(dev)
        assert rt["num_rays"] >= 24
    fq, drv = drivers()
    coarse_cfg = COARSE_CFG if with_coarse else None
    kw = driver_kwargs(name, factors, est, coarse_cfg)
    e_ref, d_max, excused, bl64, tau, excused_union = restated(model, rt, name, coarse_cfg, factors, est)
    # where coarse steps join the new depths, the excused mask goes through the driver's own join: the same call again with the mask
    # in the labels' place and zeros at the coarse steps
    joined, real_join = [], fq._join_coarse

    def join_and_mask(coarse, hit, depths_1, blidxs_1):
        assert blidxs_1.shape == excused.shape
        clean = dict(coarse, blidx=torch.zeros_like(coarse['blidx']))
        joined.append(real_join(clean, hit, depths_1, excused.to(blidxs_1.device).long())[1].bool().cpu())
        return real_join(coarse, hit, depths_1, blidxs_1)

    monkeypatch.setattr(fq, "_join_coarse", join_and_mask)
    runs = []
    for fused in (True, False):
        monkeypatch.setattr(fq, "FUSED_UPSAMPLE_FOREST", fused)
        model.sdf_block_inds.clear()
        with torch.no_grad():
            vb, det = drv[name](model, rt, **kw)
        runs.append((vb, det, model.sdf_block_inds[-1].clone()))
    (vb_f, det_f, bl_f), (vb_t, det_t, bl_t) = runs
    assert vb_f["type"] == vb_t["type"] != "empty" and set(vb_f) == set(vb_t)
    assert vb_f["type"] == ("batched" if name == "march" and not with_coarse else "packed")
    assert torch.equal(vb_f["rays_inds_hit"], vb_t["rays_inds_hit"])
    for k in ("pack_infos_hit", "num_per_hit"):
        if k in vb_t:
            assert torch.equal(torch.as_tensor(vb_f[k]), torch.as_tensor(vb_t[k])), k
    assert set(det_f) == set(det_t) and all(torch.equal(torch.as_tensor(det_f[k]), torch.as_tensor(det_t[k])) for k in det_t)
    assert vb_f["t"].shape == vb_t["t"].shape and vb_f["rgb"].shape == vb_t["rgb"].shape == (*vb_t["t"].shape, 3)
    assert vb_f["nablas"].shape == vb_f["rgb"].shape
    diff = (vb_f["t"].double() - vb_t["t"].double()).abs().max().item()
    allowed = 4 * e_ref + float(np.spacing(np.float32(d_max)))
    # labels: the last forward_sdf saw the block index of every final sample
    assert bl_f.shape == bl_t.shape
    differ = (bl_f != bl_t).cpu()
    n_ex = int(excused.sum())
    print(f"{name} coarse={with_coarse} factors={factors} est={est}: |fused - chain| {diff:.3e}  e_ref {e_ref:.3e}  allowed {allowed:.3e}; "
          f"labels: {int(differ.sum())} of {differ.numel()} differ, {n_ex} of {excused.numel()} proven ties (tau {tau:.2e})")
    assert diff <= allowed
    assert n_ex <= 0.005 * excused.numel(), "too many ties for the comparison to mean anything"
    # every label is judged, element by element; what may be excused, in the order of the samples the last forward_sdf saw:
    if name == "coarse":
        # the union behind the last stage (one factor: the reference joins nothing, the samples are the coarse steps)
        excused_all = excused_union if len(factors) > 1 else torch.zeros(bl_f.shape, dtype=torch.bool)
    elif with_coarse:
        assert len(joined) == 2
        excused_all = joined[0] | joined[1]            # coarse steps + new depths, through the join of either run
        assert int(excused_all.sum()) <= 2 * n_ex
    else:
        excused_all = excused                          # the new depths alone, [hit rays, S m] sorted as in the restatement
        if len(factors) == 1:        # one stage: the device's inputs are the restatement's, so its labels are judged against it as well
            assert not ((bl_f.cpu() != bl64) & ~excused).any(), "labels differ from the float64 restatement away from every proven tie"
    assert differ.shape == excused_all.shape, (differ.shape, excused_all.shape)
    assert not (differ & ~excused_all).any(), "labels differ away from every proven tie"
    if name == "coarse":
        # what needs no tolerance, on all 144 rays (those that pass the sphere at a distance included)
        _, _, rt_all = scene(dev)
        full = []
        for fused in (True, False):
            monkeypatch.setattr(fq, "FUSED_UPSAMPLE_FOREST", fused)
            with torch.no_grad():
                full.append(drv[name](model, rt_all, **kw))
        (vf, df), (vt, dt) = full
        assert vf["type"] == vt["type"] == "packed" and set(vf) == set(vt) and set(df) == set(dt) == {'render.num_per_ray'}
        assert torch.equal(vf["rays_inds_hit"], vt["rays_inds_hit"]) and torch.equal(vf["rays_inds_hit"], rt_all["rays_inds"])
        assert torch.equal(vf["pack_infos_hit"], vt["pack_infos_hit"]) and torch.equal(df['render.num_per_ray'], dt['render.num_per_ray'])
        assert vf["t"].shape == vt["t"].shape and torch.isfinite(vf["t"]).all() and torch.isfinite(vf["opacity_alpha"]).all()


@pytest.mark.parametrize("factors", [[1, 4, 16], [1]])
def test_one_stage_launch_per_factor(dev, monkeypatch, factors):
    from nr3d_lib_amd.bindings import _neus_upsample as U
    model, _, rt = scene(dev)
    fq, drv = drivers()
    calls, real = [], U.upsample_stage_packed_blocks

    def counted(*a, merge=True, need_sdf=True):
        calls.append((merge, need_sdf))
        return real(*a, merge=merge, need_sdf=need_sdf)

    monkeypatch.setattr(U, "upsample_stage_packed_blocks", counted)
    for name in drv:
        for fused, want in ((True, [(True, True)] * (len(factors) - 1) + [(False, False)]), (False, [])):
            monkeypatch.setattr(fq, "FUSED_UPSAMPLE_FOREST", fused)
            calls.clear()
            with torch.no_grad():
                drv[name](model, rt, **driver_kwargs(name, factors, False, None))
            assert calls == want, (name, fused)


def test_perturbed_depths_sorted_inside_the_marched_span(dev, monkeypatch):
    from nr3d_lib_amd.bindings import _neus_upsample as U
    model, _, rt = scene(dev)
    fq, drv = drivers()
    seen, real = [], U.upsample_stage_packed_blocks

    def recorded(depth, sdf, blidx, pack_infos, u, *a, **kw):
        out = real(depth, sdf, blidx, pack_infos, u, *a, **kw)
        seen.append((depth, pack_infos, u, out[0], blidx, out[1]))
        return out

    monkeypatch.setattr(U, "upsample_stage_packed_blocks", recorded)
    monkeypatch.setattr(fq, "FUSED_UPSAMPLE_FOREST", True)
    torch.manual_seed(5)
    with torch.no_grad():
        vb, _ = drv["march"](model, rt, perturb=True, march_cfg=MARCH_CFG, num_fine=8, upsample_inv_s_factors=[1, 4, 16])
    assert len(seen) == 3 and all(u.shape == (vb["t"].shape[0], 9) for _, _, u, *_ in seen), "one stratified row of u per pack"
    depth, pi = seen[0][0], seen[0][1]
    lo, hi = depth[pi[:, 0]], depth[pi[:, 0] + pi[:, 1] - 1]
    for d, p, _, fine, bl, bl_fine in seen:
        assert (fine.diff(dim=-1) >= 0).all() and (fine >= lo[:, None]).all() and (fine <= hi[:, None]).all()
        assert ((bl_fine >= 0) & (bl_fine < 7)).all(), "a new depth's block index is one of the forest's"
    assert vb["type"] == "batched" and (vb["t"].diff(dim=-1) >= 0).all()
    assert (vb["t"] >= lo[:, None]).all() and (vb["t"] <= hi[:, None]).all()


@pytest.mark.parametrize("name", ["coarse", "march", "compressed"])
def test_gradients_reach_the_radius(dev, name):
    model, _, rt = scene(dev)
    _, drv = drivers()
    model.radius.grad = None
    vb, _ = drv[name](model, rt, **driver_kwargs(name, [1, 4, 16], False, None))
    assert vb["opacity_alpha"].requires_grad
    vb["opacity_alpha"].sum().backward()
    g = model.radius.grad
    model.radius.grad = None
    assert g is not None and torch.isfinite(g) and g.abs().item() > 0


def test_no_rays_and_nothing_hit(dev):
    model, _, rt = scene(dev)
    _, drv = drivers()
    none = dict(num_rays=0, rays_inds=None)
    assert drv["coarse"](model, none) == (dict(type='empty'), {})
    assert drv["march"](model, none) == drv["compressed"](model, none) == (dict(type='empty', rays_inds_hit=[]), {})
    grid = model.accel.occ.occ_grid
    keep = grid.clone()
    grid.zero_()
    try:
        with torch.no_grad():
            for name in ("march", "compressed"):
                assert drv[name](model, rt, march_cfg=MARCH_CFG, num_fine=8) == (dict(type='empty', rays_inds_hit=[]), {})
            vb, det = drv["march"](model, rt, coarse_step_cfg=COARSE_CFG, num_fine=8)
            model.fwd_block_inds.clear()
            vb_c, det_c = drv["compressed"](model, rt, coarse_step_cfg=COARSE_CFG, num_fine=8)
    finally:
        grid.copy_(keep)
    # the coarse steps alone, with their own block indices in the final forward
    n = int(vb["pack_infos_hit"][:, 1].sum())
    assert vb["type"] == "packed" and vb["t"].shape == (n,) and vb["rgb"].shape == (n, 3) and set(det) == {'render.num_per_ray'}
    assert torch.equal(vb["rays_inds_hit"], rt["rays_inds"]) and torch.equal(det['render.num_per_ray'], vb["pack_infos_hit"][:, 1])
    assert vb_c["type"] == "packed" and set(det_c) == {'render.num_per_ray0', 'render.num_per_ray'}
    assert torch.equal(det_c['render.num_per_ray0'], vb["pack_infos_hit"][:, 1])
    assert vb_c["t"].shape[0] == int(vb_c["pack_infos_hit"][:, 1].sum()) <= n
    assert model.fwd_block_inds[-1] is not None and model.fwd_block_inds[-1].shape == vb_c["t"].shape


def test_coarse_driver_modes(dev):
    """'direct_use' and 'direct_more' (the linear stepper on the device) return the union of the steps and num_fine new depths"""
    model, _, rt = scene(dev)
    _, drv = drivers()
    with torch.no_grad():
        for mode, cfg in (('direct_use', dict()), ('direct_more', dict(step_size_nograd=0.02))):
            model.sdf_block_inds.clear()
            vb, det = drv["coarse"](model, rt, coarse_step_cfg=COARSE_CFG, upsample_mode=mode, num_fine=16, **cfg)
            pi = vb["pack_infos_hit"]
            assert vb["type"] == "packed" and torch.equal(vb["rays_inds_hit"], rt["rays_inds"]) and pi.shape == (rt["num_rays"], 2)
            assert torch.equal(det['render.num_per_ray'], pi[:, 1]) and (pi[:, 1] > 16).all()
            t = vb["t"]
            inner = torch.ones_like(t, dtype=torch.bool)
            inner[pi[:, 0] + pi[:, 1] - 1] = False
            assert (t[1:][inner[:-1]] >= t[:-1][inner[:-1]]).all(), "depths sorted per ray"
            bl = model.sdf_block_inds[-1]
            assert bl.shape == t.shape and ((bl >= 0) & (bl < 7)).all()
        with pytest.raises(RuntimeError, match="Invalid upsample_mode=cubic"):
            drv["coarse"](model, rt, upsample_mode='cubic')


def test_linear_stepper_on_the_device(dev):
    from nr3d_lib_amd.graphics.raysample import interleave_sample_step_linear_in_packed_segments
    _, _, rt = scene(dev)
    args = (rt['near'], rt['far'], rt['seg_entries'], rt['seg_exits'], rt['seg_pack_infos'])
    cfg = dict(step_size=0.07, min_steps=3, max_steps=12)
    t, dt, ridx, rpi, sidx, spi = (x.cpu().numpy() for x in interleave_sample_step_linear_in_packed_segments(*args, **cfg))
    wt, wdt, wridx, wrpi, wsidx, wspi = fref.linear_steps(*(a.cpu().numpy() for a in (args[0], *args[2:])), **cfg)
    np.testing.assert_array_equal(spi, wspi), np.testing.assert_array_equal(rpi, wrpi)
    np.testing.assert_array_equal(ridx, wridx), np.testing.assert_array_equal(sidx, wsidx)
    np.testing.assert_allclose(t, wt, rtol=0, atol=float(np.spacing(np.float32(8.0))))
    np.testing.assert_array_equal(dt, wdt)
    assert spi[:, 1].max() == 12 and (spi[:, 1] < 12).any(), "max_steps cuts some segments and not others"


@pytest.mark.parametrize("mode", ["inblock_coarse_multi_upsample", "inblock_march_occ_multi_upsample",
                                  "inblock_march_occ_multi_upsample_compressed"])
def test_mixin_ray_query_end_to_end(dev, mode):
    from nr3d_lib_amd.models.fields_forest.neus import NeuSRendererMixinForest
    base, ray_input, rt = scene(dev)

    class Net(torch.nn.Module):
        use_view_dirs = True

        def __init__(self, space):
            super().__init__()
            self.space = space

        forward_inv_s = lambda self: 256.0      # sharper than the last up-sampling stage spreads its depths: an opaque surface

        def forward_sdf(self, x, block_inds=None, block_offsets=None, input_normalized=False):
            return dict(sdf=(x - base.centre).norm(dim=-1) - 0.8)

        def forward(self, x, v=None, block_inds=None, **kw):
            return base.forward(x, v, block_inds, **kw)

    class Model(NeuSRendererMixinForest, Net):
        pass

    model = Model(space=base.space, accel=base.accel).eval()
    param = dict(upsample_mode='multistep_estimate', num_fine=16) if "coarse" in mode else dict(num_fine=8)
    cfg = dict(query_mode=mode, with_rgb=True, with_normal=True, perturb=False, query_param=param)
    with torch.no_grad():
        out = model.ray_query(ray_input=ray_input, config=cfg, return_buffer=True, return_details=True, render_per_obj_individual=True)
    n = SIDE * SIDE
    rendered, vb = out['rendered'], out['volume_buffer']
    assert vb['type'] != 'empty' and 'vw' in vb and out['details']['inv_s'] == 256.0 and 'render.num_per_ray' in out['details']
    assert rendered['mask_volume'].shape == rendered['depth_volume'].shape == (n,)
    assert rendered['rgb_volume'].shape == rendered['normals_volume'].shape == (n, 3)
    o, d = ray_input['rays_o'], ray_input['rays_d']
    closest = ((base.centre - o) - ((base.centre - o) * d).sum(-1, keepdim=True) * d).norm(dim=-1)
    through = closest < 0.6
    missed = torch.ones(n, dtype=torch.bool, device=dev)
    missed[rt['rays_inds']] = False
    assert through.sum() >= 8 and missed.sum() >= 8, "the scene has rays of both kinds"
    print(f"{mode}: mask on {int(through.sum())} rays through the sphere >= {rendered['mask_volume'][through].min().item():.4f}")
    assert (rendered['mask_volume'][through] > 0.9).all()
    assert (rendered['mask_volume'][missed] == 0).all() and (rendered['depth_volume'][missed] == 0).all()
    depth = rendered['depth_volume'][through]
    assert ((depth > 2.0) & (depth < 3.2)).all(), "the surface is met about 3 - 0.8 from the origin"
    with pytest.raises(RuntimeError, match="Invalid query_mode=march"):
        model.ray_query(ray_input=ray_input, config=dict(cfg, query_mode='march'))


def test_marched_packs_tile(dev):
    """the precondition of the stage: first_0 = 0, first_{p+1} = first_p + len_p, len_p >= 1, and the labels are the forest's blocks"""
    model, _, rt = scene(dev)
    _, _, depth, blidx, pi = loop_input(model, rt, "march", None)
    assert pi.shape[0] > 0 and pi[0, 0] == 0 and torch.equal(pi[1:, 0], (pi[:, 0] + pi[:, 1])[:-1]) and (pi[:, 1] >= 1).all()
    assert int(pi[-1].sum()) == depth.shape[0] == blidx.shape[0] and blidx.dtype == torch.int64
    assert ((blidx >= 0) & (blidx < 7)).all() and blidx.unique().numel() >= 4, "the surface lies in several blocks"
