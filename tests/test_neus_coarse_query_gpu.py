"""neus_ray_query_coarse_multi_upsample on the GPU: the fused stage inside the driver against the reference's own query
(tests/golden/ref_neus_coarse.npz) and against the torch route, and the driver's result conventions.  The model is the analytic
sphere of tests/neus_coarse_ref.py.  Values are compared under the rule of tests/test_neus_upsample_gpu.py: 4 e_ref plus one ulp,
e_ref = the distance between the float32 and float64 end-to-end runs of the restatement."""
import os

import numpy as np
import pytest
import torch

import neus_coarse_ref as ref
from nr3d_lib_amd.bindings import _neus_upsample
from nr3d_lib_amd.graphics.neus import neus_ray_query as rq
from nr3d_lib_amd.graphics.pack_ops import get_pack_infos_from_batch, packed_volume_render_compression

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_neus_coarse.npz")
QUERY = dict(upsample_mode='multistep_estimate', num_coarse=16, num_fine=8)
ULP_T, ULP_A = 2.0 ** -22, 2.0 ** -24          # one ulp of the largest depth (3.5) and of the largest opacity (1)


@pytest.fixture(scope="module")
def gold():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(GOLDEN).items()}


@pytest.fixture(scope="module")
def e_ref():
    out = {}
    for est in (False, True):
        t32, a32 = ref.coarse_query(ref.fan_rays(), 16, 8, [1, 2, 4, 8], 64., est, torch.float32)
        t64, a64 = ref.coarse_query(ref.fan_rays(), 16, 8, [1, 2, 4, 8], 64., est, torch.float64)
        out[est] = ((t32.double() - t64).abs().max().item(), (a32.double() - a64).abs().max().item())
    return out


@pytest.fixture
def stage_calls(monkeypatch):
    """the number of launches of the fused stage"""
    calls = []
    real = _neus_upsample.upsample_stage
    monkeypatch.setattr(_neus_upsample, "upsample_stage", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def _dist(a, b):
    return (a.double().cpu() - b.double().cpu()).abs().max().item()


@pytest.mark.parametrize("est", [False, True])
def test_fused_matches_reference_query(dev, gold, e_ref, stage_calls, est):
    vb, details = rq.neus_ray_query_coarse_multi_upsample(ref.SphereModel(), ref.fan_rays(device=dev), compression=False,
                                                          upsample_use_estimate_alpha=est, **QUERY)
    assert len(stage_calls) == 4, "the fused stage did not run once per up-sampling factor"
    e_t, e_a = e_ref[est]
    dt, da = _dist(vb['t'], gold[f'query_t_est{int(est)}']), _dist(vb['opacity_alpha'], gold[f'query_alpha_est{int(est)}'])
    print(f"est={est}: |t - ref| = {dt:.3e} (e_ref {e_t:.3e}), |alpha - ref| = {da:.3e} (e_ref {e_a:.3e})")
    assert vb['type'] == 'batched' and vb['t'].shape == (64, 52) and details == {'render.num_per_ray': 52}
    assert dt <= 4 * e_t + ULP_T and da <= 4 * e_a + ULP_A


@pytest.mark.parametrize("est", [False, True])
def test_fused_matches_torch_route(dev, e_ref, stage_calls, monkeypatch, est):
    kw = dict(compression=False, upsample_use_estimate_alpha=est, **QUERY)
    fused, d_fused = rq.neus_ray_query_coarse_multi_upsample(ref.SphereModel(), ref.fan_rays(device=dev), **kw)
    n_fused = len(stage_calls)
    monkeypatch.setattr(rq, "FUSED_UPSAMPLE", False)
    plain, d_plain = rq.neus_ray_query_coarse_multi_upsample(ref.SphereModel(), ref.fan_rays(device=dev), **kw)
    assert n_fused == 4 and len(stage_calls) == 4, "FUSED_UPSAMPLE = False still launched the fused stage"
    assert d_fused == d_plain and set(fused) == set(plain)
    for k in fused:
        if isinstance(fused[k], torch.Tensor):
            assert fused[k].shape == plain[k].shape and fused[k].dtype == plain[k].dtype and fused[k].device == plain[k].device, k
        else:
            assert fused[k] == plain[k], k
    dt = _dist(fused['t'], plain['t'])
    print(f"est={est}: |t fused - t torch| = {dt:.3e} (e_ref {e_ref[est][0]:.3e})")
    assert dt <= 4 * e_ref[est][0] + ULP_T


def test_compression_is_the_compaction_of_the_batched_buffer(dev):
    rays = ref.fan_rays(device=dev)
    full, _ = rq.neus_ray_query_coarse_multi_upsample(ref.SphereModel(), rays, compression=False, **QUERY)
    vb, details = rq.neus_ray_query_coarse_multi_upsample(ref.SphereModel(), rays, compression=True, **QUERY)
    alpha = full['opacity_alpha']
    nidx, pinfo, pidx = packed_volume_render_compression(alpha.flatten(), get_pack_infos_from_batch(*alpha.shape, device=dev))
    assert vb['type'] == 'packed' and 0 < pidx.numel() < alpha.numel()
    assert torch.equal(vb['rays_inds_hit'], rays['rays_inds'][nidx]) and torch.equal(vb['pack_infos_hit'], pinfo)
    for k in ('t', 'opacity_alpha'):
        assert torch.equal(vb[k], full[k].flatten()[pidx]), k
    for k in ('net_x', 'nablas', 'rgb'):
        assert torch.equal(vb[k], full[k].flatten(0, 1)[pidx]), k
    assert details['render.num_per_ray0'] == 52 and torch.equal(details['render.num_per_ray'], pinfo[:, 1])


def test_all_rays_missing_is_empty(dev):
    rays = ref.fan_rays(device=dev)
    rays['rays_d'] = -rays['rays_d']                       # looking away from the sphere
    vb, details = rq.neus_ray_query_coarse_multi_upsample(ref.SphereModel(), rays, **QUERY)
    assert vb == dict(type='empty', rays_inds_hit=[]) and details == {}


@pytest.mark.parametrize("mode,k", [('multistep_estimate', 16 + 1 + 4 * 9), ('direct_use', 16 + 1 + 8), ('direct_more', 40 + 8)])
def test_modes(dev, stage_calls, mode, k):
    model, rays = ref.SphereModel(), ref.fan_rays(device=dev)
    model.use_bidx = True
    rays['rays_bidx'] = torch.arange(64, device=dev) % 3
    kw = dict(upsample_mode=mode, num_coarse=16, num_fine=8, num_nograd=40)
    vb, details = rq.neus_ray_query_coarse_multi_upsample(model, rays, compression=False, **kw)
    assert len(stage_calls) == (4 if mode == 'multistep_estimate' else 1)
    assert vb['type'] == 'batched' and vb['num_per_hit'] == k - 1 and vb['t'].shape == vb['opacity_alpha'].shape == (64, k - 1)
    assert vb['net_x'].shape == vb['nablas'].shape == vb['rgb'].shape == (64, k - 1, 3)
    assert torch.equal(vb['rays_bidx_hit'], rays['rays_bidx']) and (vb['t'].diff(dim=-1) >= 0).all()
    packed, details = rq.neus_ray_query_coarse_multi_upsample(model, rays, **kw)
    assert packed['type'] == 'packed' and details['render.num_per_ray0'] == k - 1
    assert torch.equal(packed['rays_bidx_hit'], rays['rays_bidx'][packed['rays_inds_hit']])
    assert int(packed['pack_infos_hit'][:, 1].sum()) == packed['t'].numel() == packed['net_x'].shape[0]


def test_no_rgb_no_normal(dev):
    for compression in (False, True):
        vb, _ = rq.neus_ray_query_coarse_multi_upsample(ref.SphereModel(), ref.fan_rays(device=dev), with_rgb=False, with_normal=False,
                                                        compression=compression, **QUERY)
        assert not {'net_x', 'rgb', 'nablas'} & set(vb) and {'t', 'opacity_alpha'} <= set(vb)


def test_perturb_sorted_inside_near_far(dev, stage_calls):
    torch.manual_seed(5)
    vb, _ = rq.neus_ray_query_coarse_multi_upsample(ref.SphereModel(), ref.fan_rays(device=dev), perturb=True, compression=False, **QUERY)
    t = vb['t']
    assert len(stage_calls) == 4 and t.shape == (64, 52) and torch.isfinite(t).all()
    assert (t.diff(dim=-1) >= 0).all() and (t >= ref.NEAR).all() and (t <= ref.FAR).all()
