"""The vanilla NeuS coarse ray query without a GPU: the batched helpers and the torch route of the driver against results of the
reference's own code (tests/golden/ref_neus_coarse.npz, written by tests/golden/make_golden_neus_coarse.py), the restatement the GPU
tests measure the HIP stage against pinned to the same results, the ABI entry, and the result conventions of the driver.

Tolerances.  The helpers repeat the reference's torch expressions: a handful of float32 roundings (2^-24 relative) of values of at
most 1, carried through a sigmoid whose argument is inv_s |sdf| <= 24 * 1.5 = 36 here, so 36 * 2^-24 ~ 2e-6 covers a different
association; samples are depths of about 3, where one ulp is 2.4e-7, so 1e-6 is four of them.  The whole query is compared under the
rule of the GPU tests: 4 e_ref + one ulp, e_ref = the distance between the restatement's float32 and float64 runs."""
import os

import numpy as np
import pytest
import torch

import neus_coarse_ref as ref
from nr3d_lib_amd import _abi
from nr3d_lib_amd.graphics import raysample as rs
from nr3d_lib_amd.graphics.neus import neus_ray_query as rq
from nr3d_lib_amd.graphics.neus import neus_utils as nu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_neus_coarse.npz")
QUERY = dict(compression=False, upsample_mode='multistep_estimate', num_coarse=16, num_fine=8)
ALPHA_TOL, SAMPLE_TOL = 2e-6, 1e-6


@pytest.fixture(scope="module")
def gold():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(GOLDEN).items()}


@pytest.fixture(scope="module")
def e_ref():
    """per opacity mode: (t, alpha) of the restatement in float32 and its distance to the float64 run"""
    out = {}
    for est in (False, True):
        t32, a32 = ref.coarse_query(ref.fan_rays(), 16, 8, [1, 2, 4, 8], 64., est, torch.float32)
        t64, a64 = ref.coarse_query(ref.fan_rays(), 16, 8, [1, 2, 4, 8], 64., est, torch.float64)
        out[est] = (t32, a32, (t32.double() - t64).abs().max().item(), (a32.double() - a64).abs().max().item())
    return out


def _dist(a, b):
    return (a.double() - b.double()).abs().max().item()


def test_helpers_match_reference(gold):
    d, s = gold['h_depth'], gold['h_sdf']
    assert _dist(nu.neus_ray_sdf_to_upsample_alpha(s, d, 24.0), gold['upsample_alpha']) <= ALPHA_TOL
    assert _dist(nu.neus_ray_sdf_to_tau(s, 24.0), gold['tau']) <= 36 * ALPHA_TOL          # a log: relative to tau <= 36
    assert _dist(nu.neus_ray_sdf_to_tau(s, 24.0, append_cdf_1=True), gold['tau_append']) <= 36 * ALPHA_TOL
    assert _dist(nu.neus_ray_sdf_to_vw(s, 24.0), gold['vw']) <= ALPHA_TOL
    for ratio in (1, 0, 0.3):
        got = nu.neus_estimate_sdf_nablas_to_alpha(s, gold['h_deltas'], gold['h_nablas'], gold['h_dirs'], 24.0, ratio=ratio)
        assert _dist(got, gold[f'estimate_alpha_{ratio}']) <= ALPHA_TOL, ratio
    assert _dist(rs.batch_sample_pdf(d, gold['h_weights'], 7), gold['sample_pdf']) <= SAMPLE_TOL
    assert _dist(rs.batch_sample_cdf(d, gold['h_cdf'], 7), gold['sample_cdf']) <= SAMPLE_TOL
    assert torch.equal(rs.batch_sample_pdf(d, gold['h_weights'], 7)[3], d[3, -1].expand(7)), "a row without weight samples its last bin"


def test_helpers_differentiable():
    sdf = torch.linspace(1.0, -1.0, 9).expand(2, 9).clone().requires_grad_()
    (nu.neus_ray_sdf_to_vw(sdf, 8.0).sum() + nu.neus_ray_sdf_to_tau(sdf, 8.0).sum() + nu.neus_pdf(sdf, 8.0).sum()).backward()
    assert torch.isfinite(sdf.grad).all() and sdf.grad.abs().sum() > 0
    assert torch.allclose(nu.neus_pdf(torch.zeros(1), 8.0), torch.tensor([2.0]))        # inv_s / 4 at the surface


def test_perturbed_samples_sorted_inside_bins(gold):
    torch.manual_seed(3)
    t = rs.batch_sample_pdf(gold['h_depth'], gold['h_weights'], 33, perturb=True)
    assert t.shape == (5, 33) and (t.diff(dim=-1) >= 0).all()
    assert (t >= gold['h_depth'][:, :1]).all() and (t <= gold['h_depth'][:, -1:]).all()


@pytest.mark.parametrize("est", [False, True])
def test_torch_route_matches_reference_query(gold, e_ref, est):
    vb, details = rq.neus_ray_query_coarse_multi_upsample(ref.SphereModel(), ref.fan_rays(), upsample_use_estimate_alpha=est, **QUERY)
    _, _, e_t, e_a = e_ref[est]
    dt, da = _dist(vb['t'], gold[f'query_t_est{int(est)}']), _dist(vb['opacity_alpha'], gold[f'query_alpha_est{int(est)}'])
    print(f"est={est}: |t - ref| = {dt:.3e} (e_ref {e_t:.3e}), |alpha - ref| = {da:.3e} (e_ref {e_a:.3e})")
    assert vb['t'].shape == (64, 52) and details == {'render.num_per_ray': 52}
    assert dt <= 4 * e_t + 2.0 ** -22 and da <= 4 * e_a + 2.0 ** -24


@pytest.mark.parametrize("est", [False, True])
def test_restatement_matches_reference_query(gold, e_ref, est):
    t32, a32, e_t, e_a = e_ref[est]
    dt, da = _dist(t32, gold[f'query_t_est{int(est)}']), _dist(a32, gold[f'query_alpha_est{int(est)}'])
    print(f"est={est}: |t - ref| = {dt:.3e} (e_ref {e_t:.3e}), |alpha - ref| = {da:.3e} (e_ref {e_a:.3e})")
    assert dt <= 4 * e_t + 2.0 ** -22 and da <= 4 * e_a + 2.0 ** -24


def test_abi_lists_the_stage():
    assert _abi.ABI_VERSION >= 17
    ret, args = _abi.SIGNATURES['nr3d_neus_upsample_stage']
    assert ret == 'int' and args == ['uint32_t'] * 3 + ['ptr'] * 3 + ['int64_t', 'float', 'int'] + ['ptr'] * 4
    assert _abi.SIGNATURES['nr3d_neus_upsample_max_row'] == ('int', [])
    assert 'neus_ray_query_coarse_multi_upsample' in rq.__all__


@pytest.mark.parametrize("mode,k", [('multistep_estimate', 16 + 1 + 4 * 9), ('direct_use', 16 + 1 + 8), ('direct_more', 40 + 8)])
def test_result_conventions(mode, k):
    rays = ref.fan_rays(3)
    vb, details = rq.neus_ray_query_coarse_multi_upsample(ref.SphereModel(), rays, compression=False, upsample_mode=mode,
                                                          num_coarse=16, num_fine=8, num_nograd=40, chunksize_query=4)
    assert vb['type'] == 'batched' and vb['num_per_hit'] == k - 1 and details == {'render.num_per_ray': k - 1}
    assert set(vb) == {'type', 'rays_inds_hit', 'num_per_hit', 't', 'opacity_alpha', 'net_x', 'nablas', 'rgb'}
    assert vb['t'].shape == vb['opacity_alpha'].shape == (9, k - 1)
    assert vb['net_x'].shape == vb['nablas'].shape == vb['rgb'].shape == (9, k - 1, 3)
    assert torch.equal(vb['rays_inds_hit'], rays['rays_inds'])
    assert (vb['t'].diff(dim=-1) >= 0).all() and (vb['t'] >= ref.NEAR).all() and (vb['t'] <= ref.FAR).all()
    bare, _ = rq.neus_ray_query_coarse_multi_upsample(ref.SphereModel(), rays, with_rgb=False, with_normal=False, compression=False,
                                                      upsample_mode=mode, num_coarse=16, num_fine=8, num_nograd=40)
    assert set(bare) == {'type', 'rays_inds_hit', 'num_per_hit', 't', 'opacity_alpha'} and torch.equal(bare['t'], vb['t'])


def test_bidx_and_invalid_mode():
    model, rays = ref.SphereModel(), ref.fan_rays(2)
    model.use_bidx = True
    rays['rays_bidx'] = torch.arange(4)
    vb, _ = rq.neus_ray_query_coarse_multi_upsample(model, rays, compression=False, num_coarse=8, num_fine=4)
    assert torch.equal(vb['rays_bidx_hit'], rays['rays_bidx'])
    with pytest.raises(RuntimeError, match="Invalid upsample_mode"):
        rq.neus_ray_query_coarse_multi_upsample(model, rays, compression=False, upsample_mode='nope')


def test_no_rays_is_empty():
    vb, details = rq.neus_ray_query_coarse_multi_upsample(ref.SphereModel(), dict(num_rays=0))
    assert vb == dict(type='empty', rays_inds_hit=[]) and details == {}
