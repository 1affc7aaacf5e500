"""The forest NeuS ray queries without a GPU: the label-carrying restatement (tests/neus_forest_ref.py) on hand-built packs, the linear
stepper of graphics.raysample against a plain loop, the refusals of the new binding, and the dispatch of NeuSRendererMixinForest.

The stepper is built from pack ops that run on the GPU only.  Here it runs on CPU tensors with three of them replaced by torch
stand-ins (interleave_arange_simple, interleave_linstep, packed_diff), so what is checked is the stepper's own arithmetic: the
rungs, the clamps and the packs.  tests/test_neus_forest_query_gpu.py runs it on the real ops against the same loop."""
import numpy as np
import pytest
import torch

import neus_coarse_ref as cref
import neus_forest_ref as fref
import neus_packed_ref as ref
from nr3d_lib_amd import _abi
from nr3d_lib_amd.graphics.neus import neus_forest_ray_query as fq      # the feature under test: without it nothing here runs


# ---- the restatement ------------------------------------------------------------------------------------------------------------

def step_pack(n, k_star, spacing=0.05):
    """depths i * spacing, SDF +100 up to k_star and -100 after it: both sigmoids of interval k_star are exactly 1 and 0 (or the one
    weight is the only one), so the CDF is exactly 0 up to k_star and exactly 1 after, in any precision"""
    d = torch.arange(n, dtype=torch.float32) * spacing + 1.0
    s = torch.where(torch.arange(n) <= k_star, torch.tensor(100.0), torch.tensor(-100.0))
    return d, s


@pytest.mark.parametrize("est", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_step_pack_has_an_exact_cdf(est, dtype):
    n, k = 9, 4
    d, s = step_pack(n, k)
    bl = torch.where(torch.arange(n) <= k, 7, 9)
    pi = torch.tensor([[0, n]])
    u = cref.shared_u(5)
    r = fref.stage(d, s, bl, pi, u, 64.0, est, dtype)
    assert torch.equal(r['cdf'], (torch.arange(n) > k).to(dtype))
    assert torch.equal(r['pos'], torch.full((1, 5), k + 1)) and torch.equal(r['blidx_fine'], torch.full((1, 5), 9))
    want = d[k].to(dtype) + u.to(dtype) * (d[k + 1] - d[k]).to(dtype)
    assert torch.allclose(r['fine'][0], want, rtol=0, atol=1e-6)
    # the union: new depths lie strictly inside (d_k, d_k+1), so they follow sample k
    assert r['blidx_merged'].tolist() == [7] * (k + 1) + [9] * 5 + [9] * (n - k - 1)
    assert r['pidx_fine'].tolist() == [list(range(k + 1, k + 6))]


def test_labels_follow_pos_not_the_raised_depth():
    """two packs by hand: a pack of one element (pos = 0 for every u) and a pack without mass (pos = n - 1: no knot reaches u, the
    depth comes from n - 2 by the pmf rule, the label from n - 1)"""
    d = torch.tensor([2.0, 1.0, 1.5, 2.0, 2.5])
    s = torch.tensor([0.3, 5.0, 5.0, 5.0, 5.0])
    bl = torch.tensor([11, 20, 21, 22, 2 ** 40 + 5])
    pi = torch.tensor([[0, 1], [1, 4]])
    r = fref.stage(d, s, bl, pi, cref.shared_u(3), 64.0, False, torch.float64)
    assert r['pos'].tolist() == [[0, 0, 0], [3, 3, 3]]
    assert r['blidx_fine'].tolist() == [[11] * 3, [2 ** 40 + 5] * 3]
    assert r['fine'].tolist() == [[2.0] * 3, [2.0] * 3]                      # depth_{n-2}: the pmf is 0
    # a new depth goes before an equal old one: 2.0 x3 then the old 2.0
    assert r['blidx_merged'].tolist() == [11] * 3 + [11] + [20, 21] + [2 ** 40 + 5] * 3 + [22, 2 ** 40 + 5]
    assert torch.equal(r['blidx_merged'][r['pidx_fine']], r['blidx_fine'])


@pytest.mark.parametrize("est", [False, True])
def test_restatement_adds_to_the_packed_one_and_ties_are_rare(est):
    """on the parity inputs of the GPU test: the added `pos` reproduces neus_packed_ref's `fine` (same CDF, same bin), the float32 and
    the float64 run find the same bins, and few cases lie within tau of a knot"""
    n_cases = n_ties = n_differ = 0
    worst = 0.0
    for m in ref.PARITY_M:
        depth, sdf, pi = ref.sphere_packs(ref.parity_lengths(512, m))
        bl = fref.labels_every(pi)
        u = cref.shared_u(m)
        for inv_s in ref.PARITY_INV_S:
            r32 = fref.stage(depth, sdf, bl, pi, u, float(inv_s), est, torch.float32)
            r64 = fref.stage(depth, sdf, bl, pi, u, float(inv_s), est, torch.float64)
            for r, dt in ((r32, torch.float32), (r64, torch.float64)):
                for p, (b, n) in enumerate(pi.tolist()):
                    pos, lo = r['pos'][p], (r['pos'][p] - 1).clamp_min(0)
                    c, d = r['cdf'][b:b + n], depth[b:b + n].to(dt)
                    pmf = c[pos] - c[lo]
                    lerp = ref._fma((u.to(dt) - c[lo]) / torch.where(pmf < ref.PMF_MIN, torch.ones_like(pmf), pmf), d[pos] - d[lo], d[lo])
                    fine = torch.where(pos == 0, d[0].expand_as(lerp), torch.where(pmf < ref.PMF_MIN, d[lo], lerp))
                    assert torch.equal(torch.cummax(fine, 0).values, r['fine'][p]), f"pack {p}: pos does not reproduce fine"
            tau = fref.cdf_tau(r32, r64)
            worst = max(worst, tau / 4)
            ties = fref.proven_ties(r64['cdf'], pi, u, tau)
            differ = r32['pos'] != r64['pos']
            assert not (differ & ~ties).any(), "float32 and float64 disagree on a bin away from every knot"
            n_cases, n_ties, n_differ = n_cases + ties.numel(), n_ties + int(ties.sum()), n_differ + int(differ.sum())
    print(f"est={est}: {n_cases} cases, {n_ties} proven ties, {n_differ} positions differ, largest |cdf32 - cdf64| {worst:.2e}")
    assert n_ties <= 0.005 * n_cases


def test_loop_restatement_matches_the_packed_one():
    rays = cref.fan_rays(4)
    lengths = [17, 33, 5, 64]
    depth, _, pi = ref.sphere_packs(lengths)
    o, v = rays['rays_o'][:4], rays['rays_d'][:4]
    bl = fref.labels_every(pi)
    u = cref.shared_u(9, torch.float64)                  # as neus_packed_ref.upsample_loop draws it
    out = fref.upsample_loop(lambda x: x.norm(dim=-1) - cref.RADIUS, o, v, depth, bl, pi, 8, [1, 4, 16], 64.0, False, u, torch.float64,
                             ties=True)
    want = ref.upsample_loop(o, v, depth, pi, 8, [1, 4, 16], 64.0, False, torch.float64)
    assert torch.equal(out['fine'], want)
    assert out['blidx'].shape == out['excused'].shape == want.shape and len(out['taus']) == 3 and max(out['taus']) < 1e-3
    assert out['excused'].sum() <= 2, "ties are rare on these packs"
    assert out['excused_union'].shape == (depth.shape[0] + 4 * 27,) and out['excused_union'].sum() == out['excused'].sum()
    first = {p: 1000 * p for p in range(4)}
    assert all(((out['blidx'][p] >= first[p]) & (out['blidx'][p] < first[p] + 1000)).all() for p in range(4)), "a label left its pack"


# ---- the linear stepper ---------------------------------------------------------------------------------------------------------

def _cpu_pack_ops(monkeypatch):
    from nr3d_lib_amd.graphics import raysample

    def interleave_arange_simple(stop, return_idx=True):
        idx = torch.repeat_interleave(torch.arange(stop.shape[0]), stop)
        first = torch.cumsum(stop, 0) - stop
        return torch.arange(idx.shape[0]) - first[idx], idx

    def interleave_linstep(start, num_steps, step_size, return_idx=True):
        k, idx = interleave_arange_simple(num_steps)
        return start[idx] + k * step_size, idx

    def packed_diff(feats, pack_infos):
        out = torch.zeros_like(feats)
        out[:-1] = feats[1:] - feats[:-1]
        out[pack_infos[:, 0] + pack_infos[:, 1] - 1] = 0
        return out

    for name, fn in (("interleave_arange_simple", interleave_arange_simple), ("interleave_linstep", interleave_linstep),
                     ("packed_diff", packed_diff)):
        monkeypatch.setattr(raysample, name, fn)
    return raysample


# two rays; segments: ordinary, shorter than one step (min_steps), far longer than max_steps allows, ordinary
NEAR = torch.tensor([0.5, 1.25])
SEG_PACK_INFOS = torch.tensor([[0, 3], [3, 1]])
ENTRY = torch.tensor([0.503, 1.013, 2.007, 1.251])
EXIT = torch.tensor([0.957, 1.015, 9.004, 1.404])


@pytest.mark.parametrize("kw", [dict(), dict(step_size=0.02, step_size_factor=2.0), dict(min_steps=4, max_steps=16)])
def test_linear_stepper_against_the_plain_loop(monkeypatch, kw):
    rs = _cpu_pack_ops(monkeypatch)
    cfg = dict(step_size=0.05, step_size_factor=1.0, min_steps=2, max_steps=32)
    cfg.update(kw)
    t, dt, ridx, rpi, sidx, spi = rs.interleave_sample_step_linear_in_packed_segments(NEAR, 100.0, ENTRY, EXIT, SEG_PACK_INFOS, **cfg)
    wt, wdt, wridx, wrpi, wsidx, wspi = fref.linear_steps(NEAR.numpy(), ENTRY.numpy(), EXIT.numpy(), SEG_PACK_INFOS.numpy(), **cfg)
    np.testing.assert_array_equal(spi.numpy(), wspi)
    np.testing.assert_array_equal(rpi.numpy(), wrpi)
    np.testing.assert_array_equal(ridx.numpy(), wridx)
    np.testing.assert_array_equal(sidx.numpy(), wsidx)
    np.testing.assert_allclose(t.numpy(), wt, rtol=0, atol=float(np.spacing(np.float32(9.0))))
    np.testing.assert_array_equal(dt.numpy(), wdt)
    n = spi[:, 1].tolist()
    assert n[1] == cfg['min_steps'] and n[2] == cfg['max_steps'], "the short segment is raised to min_steps, the long one cut at max_steps"
    step = cfg['step_size'] * cfg['step_size_factor']
    assert n[0] == int((0.957 - 0.5) / step) - int((0.503 - 0.5) / step) + 1
    assert rpi.tolist() == [[0, sum(n[:3])], [sum(n[:3]), n[3]]]
    # every segment starts on the last rung at or below its entry
    first = t[spi[:, 0]]
    assert (first <= ENTRY + 1e-6).all() and (first > ENTRY - step - 1e-6).all()


def test_linear_stepper_perturbed(monkeypatch):
    rs = _cpu_pack_ops(monkeypatch)
    torch.manual_seed(3)
    t, dt, ridx, rpi, sidx, spi = rs.interleave_sample_step_linear_in_packed_segments(NEAR, 100.0, ENTRY, EXIT, SEG_PACK_INFOS,
                                                                                       step_size=0.05, max_steps=32, perturb=True)
    plain = rs.interleave_sample_step_linear_in_packed_segments(NEAR, 100.0, ENTRY, EXIT, SEG_PACK_INFOS, step_size=0.05, max_steps=32)
    assert spi[0, 1] == plain[5][0, 1] - 1, "perturbed: one rung fewer, the last sample stays below the exit's rung"
    last = spi[:, 0] + spi[:, 1] - 1
    inner = torch.ones_like(t, dtype=torch.bool)
    inner[last] = False
    assert (dt[inner] > 0).all() and (dt[inner] < 0.1).all() and torch.equal(dt[last], torch.full((4,), 0.05))
    assert torch.allclose(t[1:][inner[:-1]] - t[:-1][inner[:-1]], dt[inner])


def test_ray_step_coarse_modes(monkeypatch):
    from nr3d_lib_amd.models.spatial import forest
    seen = []

    class Reached(Exception):
        pass

    def stepper(*a, **kw):
        seen.append(kw)
        raise Reached

    monkeypatch.setattr(forest, "interleave_sample_step_linear_in_packed_segments", stepper)
    space = forest.ForestBlockSpace()
    with pytest.raises(Reached):
        space.ray_step_coarse(None, None, None, None, None, None, None, None, step_mode='linear', step_size=0.2)
    assert seen == [dict(step_size=0.2)]
    with pytest.raises(RuntimeError, match="Invalid step_mode=cubic"):
        space.ray_step_coarse(None, None, None, None, None, None, None, None, step_mode='cubic')


# ---- the binding ----------------------------------------------------------------------------------------------------------------

def test_abi_lists_the_blocks_stage():
    assert _abi.ABI_VERSION >= 27
    # the labelled argument list, under the one packed entry's name since ABI 28: the unlabelled call passes NULL for the three
    ret, args = _abi.SIGNATURES['nr3d_neus_upsample_stage_packed']
    assert ret == 'int' and args == ['uint32_t', 'uint64_t', 'uint32_t'] + ['ptr'] * 5 + ['int64_t', 'float', 'int', 'int', 'int'] \
        + ['ptr'] * 8 + ['ptr']
    assert 'nr3d_neus_upsample_stage_packed_blocks' not in _abi.SIGNATURES


def test_binding_refuses_cpu_tensors_and_non_tensors():
    from nr3d_lib_amd.bindings import _neus_upsample as U
    depth, sdf, pi = ref.sphere_packs([17, 5])
    bl = fref.labels_every(pi)
    with pytest.raises(RuntimeError, match="GPU only"):
        U.upsample_stage_packed_blocks(depth, sdf, bl, pi, cref.shared_u(9), 64.0, False)
    with pytest.raises(RuntimeError, match="`depth` must be a tensor"):
        U.upsample_stage_packed_blocks(depth.numpy(), sdf, bl, pi, cref.shared_u(9), 64.0, False)
    assert "upsample_stage_packed_blocks" in U.__all__


# ---- the mixin ------------------------------------------------------------------------------------------------------------------

class _Space:
    def __init__(self, num_rays):
        self.num_rays, self.calls = num_rays, []

    def ray_test(self, rays_o, rays_d, near=None, far=None, return_rays=True, **extra):
        self.calls.append((near, far, return_rays, sorted(extra)))
        n = self.num_rays
        return dict(num_rays=n, rays_inds=torch.arange(n) if n else None, rays_o=rays_o[:n], rays_d=rays_d[:n])


class _Net:
    use_view_dirs = False

    def __init__(self, space=None):
        self.space = space

    def forward_inv_s(self):
        return torch.tensor(32.0)

    def forward_sdf(self, x, block_inds=None, block_offsets=None, input_normalized=False):
        return dict(sdf=x.norm(dim=-1) - 0.5, seen=(block_inds, input_normalized))

    def forward_sdf_nablas(self, x, block_inds=None, block_offsets=None, input_normalized=False):
        return dict(sdf=x.norm(dim=-1) - 0.5, nablas=x)


def _model(num_rays, **kw):
    from nr3d_lib_amd.models.fields_forest.neus import NeuSRendererMixinForest

    class Model(NeuSRendererMixinForest, _Net):
        pass

    return Model(space=_Space(num_rays), **kw), NeuSRendererMixinForest


def test_mixin_construction_and_forward_sdf():
    model, mixin = _model(0, ray_query_cfg=dict(a=1), accel_cfg=dict(type='occ_grid_forest'))
    assert model.ray_query_cfg == dict(a=1) and model.accel is None and model.upsample_s_divisor == 1.0
    with pytest.raises(AssertionError):
        mixin()

    class Accel:
        got = None

        def collect_samples(self, x, blidx, val, normalized=True):
            self.got = (x.shape, blidx, val.shape, normalized)

    model.accel = Accel()
    x, b = torch.rand(5, 3), torch.arange(5)
    out = model.forward_sdf(x, b)
    assert out['seen'][0] is b and out['seen'][1] is False and model.accel.got == (x.shape, b, (5,), False)
    model.accel.got = None
    model.forward_sdf(x, b, skip_accel=True, input_normalized=True)
    assert model.accel.got is None


def test_mixin_empty_rays_and_dispatch(monkeypatch):
    from nr3d_lib_amd.models.fields_forest.neus import renderer_mixin as rm
    model, _ = _model(0)
    rays = dict(rays_o=torch.zeros(2, 3, 3), rays_d=torch.ones(2, 3, 3))
    with pytest.raises(AssertionError, match=r"\[N, 3\]"):
        model.ray_test(**rays)
    rays = dict(rays_o=torch.zeros(6, 3), rays_d=torch.ones(6, 3), near=0.1, far=4.0)
    cfg = dict(query_mode='nonsense', with_rgb=True, with_normal=True, perturb=False, query_param=dict(num_fine=4))
    out = model.ray_query(ray_input=rays, config=cfg, return_buffer=True, return_details=True, render_per_obj_individual=True)
    assert model.space.calls == [(0.1, 4.0, True, [])]
    assert out['volume_buffer'] == dict(type='empty', rays_inds_hit=[])
    assert out['details']['inv_s'] == 32.0 and out['details']['s'] == 1 / 32.0
    assert sorted(out['rendered']) == ['depth_volume', 'mask_volume', 'normals_volume', 'rgb_volume']
    assert out['rendered']['mask_volume'].shape == (6,) and out['rendered']['rgb_volume'].shape == (6, 3)
    assert not any(v.any() for v in out['rendered'].values())
    assert model.ray_query(ray_input=rays, config=cfg) == {}

    # with rays: the mode picks the driver; an unknown one raises
    model, _ = _model(4)
    with pytest.raises(RuntimeError, match="Invalid query_mode=nonsense"):
        model.ray_query(ray_input=rays, config=cfg)
    seen = []
    for mode in list(rm._QUERY_MODES):
        def fake(m, ray_tested, _mode=mode, **kw):
            seen.append((_mode, ray_tested['num_rays'], kw))
            return dict(type='empty', rays_inds_hit=[]), {'render.num_per_ray': 0}
        monkeypatch.setitem(rm._QUERY_MODES, mode, fake)
    assert sorted(rm._QUERY_MODES) == ['inblock_coarse_multi_upsample', 'inblock_march_occ_multi_upsample',
                                       'inblock_march_occ_multi_upsample_compressed']

    class Cfg:                                           # attribute access works as dict access does
        with_rgb, with_normal, perturb, forward_inv_s, query_param = False, True, True, 48.0, dict(num_fine=4)

    for mode in sorted(rm._QUERY_MODES):
        Cfg.query_mode = mode
        out = model.ray_query(ray_input=rays, config=Cfg, return_details=True, render_per_obj_individual=True)
        assert seen[-1] == (mode, 4, dict(with_rgb=False, with_normal=True, perturb=True, forward_inv_s=48.0, num_fine=4))
        assert out['details']['render.num_per_ray'] == 0 and out['details']['inv_s'] == 48.0
        assert sorted(out['rendered']) == ['depth_volume', 'mask_volume', 'normals_volume']


def test_drivers_return_empty_without_rays():
    from nr3d_lib_amd.graphics import neus as N
    assert N.neus_forest_ray_query_coarse_multi_upsample is fq.neus_forest_ray_query_coarse_multi_upsample
    model, _ = _model(0)
    rt = dict(num_rays=0, rays_inds=None)
    assert N.neus_forest_ray_query_coarse_multi_upsample(model, rt) == (dict(type='empty'), {})
    for fn in (N.neus_forest_ray_query_march_occ_multi_upsample, N.neus_forest_ray_query_march_occ_multi_upsample_compressed):
        assert fn(model, rt) == (dict(type='empty', rays_inds_hit=[]), {})
