"""The NeRF++ distant-view sampler: every ray against concentric shells around the close-range box, the valid samples packed with their
4-D network input -- counterpart of ``NeRFRendererMixinDistant._ray_marching`` (nr3d_lib/models/fields_distant/nerf/
renderer_mixin.py:170-288) and of the two intersection helpers in front of it (:31-82).

Two routes, same results up to rounding (tests/test_nerfpp_march_gpu.py):
  * the torch route: the reference's chain, op for op -- dense [num_rays, N (+ 1)] tensors, nonzero(), four gathers, a second nonzero();
  * the fused route (``bindings._nerfpp_march``, csrc/nerfpp_march.hip): count, one scan with the ONE device->host readback, emit.  It
    builds the SAME 1-D table of shell radii with the same ``torch.arange`` call and, with ``perturb``, draws the same
    ``torch.rand([num_rays, N])`` from the same generator state, so un-perturbed radii are bit-identical and a fixed seed gives both
    routes the same noise.  N is whatever ``arange`` returns, NOT ``max_steps``: radius_scale_min=1, radius_scale_max=100,
    max_steps=100 gives 101 inverse-proportional shells (and 100 logarithmic ones).
The kernel has NO backward: the fused route serves float32 GPU rays that do not require grad; everything else (CPU tensors, other
dtypes, ``rays_o`` / ``rays_d`` that require grad, ``fused=False``) takes the torch route."""
import math
from collections import namedtuple
from typing import Optional, Union

import numpy as np
import torch
import torch.nn.functional as F

from nr3d_lib_amd.bindings import _nerfpp_march
from nr3d_lib_amd.graphics.pack_ops import get_pack_infos_from_n
from nr3d_lib_amd.models.spatial import AABBSpace

__all__ = ['ray_sphere_intersect', 'ray_box_intersect', 'nerfpp_raymarch_ret', 'nerfpp_raymarch', 'FUSED_NERFPP_MARCH']

# True: float32 GPU rays without grad go through the HIP kernels; False (and every other input): the reference's op chain.
# Default by profiles/nerfpp_march.json (tools/exp_nerfpp_march.py): True only while the fused route is not slower in any row.
FUSED_NERFPP_MARCH = True

nerfpp_raymarch_ret = namedtuple("nerfpp_raymarch_ret", "ridx_hit samples depth_samples deltas ridx pack_infos")

_SAMPLE_MODES = dict(box='box', fixed_cuboid_shells='box', ellipsoid='ellipsoid', fixed_ellipsoid_shells='ellipsoid',
                     cube='cube', fixed_cubic_shells='cube', spherical='spherical', fixed_spherical_shells='spherical')
_LINDISP = ('lindisp', 'moving_spherical_shells')
_RETIRED = ('moving_far_spherical', 'neurecon01', 'neurecon02')
_INTERVAL_TYPES = ('inverse_proportional', 'logarithm', 'logarithm_with_inverse_prop_input')


def ray_sphere_intersect(rays_o: torch.Tensor, rays_d: torch.Tensor, r: Union[float, torch.Tensor]) -> torch.Tensor:
    """rays_o, rays_d [B, 3], r [(B,) P] radii -> [B, P] depth of the far crossing of every sphere; NaN where the ray misses it"""
    p = rays_o.unsqueeze(1)
    v = rays_d.unsqueeze(1)
    pp = (p * p).sum(dim=2)
    vv = (v * v).sum(dim=2)
    pv = (p * v).sum(dim=2)
    return ((pv * pv - vv * (pp - r * r)).sqrt() - pv) / vv


def ray_box_intersect(rays_o: torch.Tensor, rays_d: torch.Tensor, r: Union[float, torch.Tensor]) -> torch.Tensor:
    """rays_o, rays_d [B, 3], r [(B,) P] half side lengths -> [B, P] depth of the far crossing of every box; NaN where the ray misses it
    or the box lies behind the origin"""
    rays_o = rays_o.unsqueeze(1)
    rays_d = rays_d.unsqueeze(1)
    r = r[..., None]
    t_min = (-r - rays_o) / rays_d
    t_max = (r - rays_o) / rays_d
    t_near = torch.minimum(t_min, t_max).max(dim=-1).values
    t_far = torch.maximum(t_min, t_max).min(dim=-1).values
    mask_intersect = (t_far > t_near) & (t_far > 0)
    t_far[~mask_intersect] = math.nan
    return t_far


def _shell_table(radius_scale_min, radius_scale_max, max_steps, interval_type, device):
    """the chain's 1-D table: (radii [N] -- 1 / r or log10 r --, step, log10 r_min, log10 r_max)"""
    if interval_type == 'inverse_proportional':
        start, end = 1. / radius_scale_min, 1. / radius_scale_max
        log_min = log_max = None
    else:
        start, end = log_min, log_max = np.log10(radius_scale_min), np.log10(radius_scale_max)
    step_size = (end - start) / max_steps
    return torch.arange(start, end, step_size, device=device), step_size, log_min, log_max


def _torch_route(space, rays_o, rays_d, t_min, radius_scale_max, include_inf_distance, perturb, sample_mode, interval_type, table):
    radii, step_size, log_min, log_max = table
    num_rays = rays_o.shape[0]
    device, dtype = rays_o.device, rays_o.dtype
    if interval_type == 'inverse_proportional':
        r_reci = radii.expand(num_rays, -1)
        if perturb:
            r_reci = (r_reci + torch.rand_like(r_reci) * step_size).clamp(1e-5)
        r = r_reci.reciprocal()
    else:
        r_log = radii.expand(num_rays, -1)
        if perturb:
            r_log = r_log + torch.rand_like(r_log) * step_size
        r = 10 ** r_log
        r_reci = r.reciprocal()
    r_extended = torch.cat([r, torch.full([num_rays, 1], 1.0e10 if include_inf_distance else radius_scale_max, device=device,
                                          dtype=dtype)], dim=-1)
    stretch = space.aabb[1] - space.aabb[0]
    rays_o_normed, rays_d_normed = space.normalize_rays(rays_o, rays_d)

    if sample_mode in ('box', 'ellipsoid'):
        intersect = ray_box_intersect if sample_mode == 'box' else ray_sphere_intersect
        t_extended = intersect(rays_o_normed, rays_d_normed, r_extended)
        deltas = t_extended.diff(dim=-1)
        t = t_extended[:, :-1]
        x = torch.addcmul(rays_o_normed.unsqueeze(-2), rays_d_normed.unsqueeze(-2), t.unsqueeze(-1))
        norm_is_radius = True
    else:
        # the shortest side of the box is the side of the cube / the radius of the sphere
        intersect = ray_box_intersect if sample_mode == 'cube' else ray_sphere_intersect
        t_extended = intersect(rays_o, rays_d, r_extended * stretch.min())
        deltas = t_extended.diff(dim=-1)
        t = t_extended[:, :-1]
        x = space.normalize_coords(torch.addcmul(rays_o.unsqueeze(-2), rays_d.unsqueeze(-2), t.unsqueeze(-1)))
        norm_is_radius = False

    x_dir = x * r_reci.unsqueeze(-1) if norm_is_radius else F.normalize(x, dim=-1)
    if interval_type in ('inverse_proportional', 'logarithm_with_inverse_prop_input'):
        x_norm_reci = r_reci if norm_is_radius else x.norm(dim=-1).reciprocal()
        r_in_net = x_norm_reci.unsqueeze(-1) * 2. - 1
    else:
        x_norm_log = r_log if norm_is_radius else torch.log10(x.norm(dim=-1))
        r_in_net = (x_norm_log.unsqueeze(-1) - log_min) / (log_max - log_min) * 2 - 1.
    x = torch.cat([x_dir, r_in_net], dim=-1)                  # [num_rays, N, 4]: the NeRF++ input in grid coordinates [-1, 1]

    valid_samples = ~(torch.isnan(t) | (t < t_min[:, None]))
    ridx, pidx = valid_samples.nonzero().long().t()
    if ridx.numel() == 0:
        return nerfpp_raymarch_ret(None, None, None, None, None, None)
    pack_infos = get_pack_infos_from_n(valid_samples.sum(-1))
    ridx_hit = pack_infos[..., 1].nonzero().long()[..., 0].contiguous()
    pack_infos = pack_infos[ridx_hit].contiguous().long()
    return nerfpp_raymarch_ret(ridx_hit, x[ridx, pidx], t[ridx, pidx], deltas[ridx, pidx], ridx, pack_infos)


def nerfpp_raymarch(space, rays_o: torch.Tensor, rays_d: torch.Tensor, t_min: torch.Tensor, t_max: Optional[torch.Tensor] = None, *,
                    radius_scale_min: float = 1.0, radius_scale_max: float = 100.0, include_inf_distance: bool = None,
                    perturb: bool = False, max_steps: int = 256, sample_mode: str = 'box',
                    interval_type: str = 'inverse_proportional', fused: Optional[bool] = None) -> nerfpp_raymarch_ret:
    """rays_o, rays_d [num_rays, 3] in the object space of ``space`` (an AABBSpace: the close-range box), t_min [num_rays]: shells
    closer than it are dropped (``t_max`` is accepted and unused, as in the reference).  -> nerfpp_raymarch_ret(ridx_hit [P'], samples
    [S, 4], depth_samples [S], deltas [S], ridx [S], pack_infos [P', 2]) in (ray, shell) order, or six ``None`` without a valid sample.

    sample_mode: 'box' | 'ellipsoid' (shells of the box's proportions, radius = norm in normalised space), 'cube' | 'spherical' (regular
    shells sized by the box's shortest side), and the reference's long names for them.  interval_type: 'inverse_proportional',
    'logarithm', 'logarithm_with_inverse_prop_input'.  ``fused``: None = the module switch FUSED_NERFPP_MARCH, False = the torch route;
    the fused route has no backward and takes float32 GPU rays that do not require grad only (module docstring)."""
    if sample_mode in _LINDISP:
        raise RuntimeError(f"sample_mode={sample_mode} cannot run: the reference's branch never defines `deltas` and fails with "
                           "UnboundLocalError; it is refused here on both routes")
    if sample_mode in _RETIRED:
        raise RuntimeError(f"sample_mode={sample_mode} no longer supported.")
    if sample_mode not in _SAMPLE_MODES:
        raise RuntimeError(f"Invalid sample_mode={sample_mode}")
    if interval_type not in _INTERVAL_TYPES:
        raise RuntimeError(f"Invalid interval_type={interval_type}")
    if not isinstance(space, AABBSpace):
        raise NotImplementedError(f"Not supported inner boundary space type={type(space)}")
    mode = _SAMPLE_MODES[sample_mode]
    table = _shell_table(radius_scale_min, radius_scale_max, max_steps, interval_type, rays_o.device)
    use_fused = FUSED_NERFPP_MARCH if fused is None else fused
    aabb = space.aabb
    if use_fused and not (rays_o.is_cuda and rays_d.is_cuda and t_min.is_cuda and aabb.is_cuda
                          and rays_o.dtype == rays_d.dtype == t_min.dtype == aabb.dtype == torch.float32
                          and rays_o.dim() == 2 and not (torch.is_grad_enabled() and (rays_o.requires_grad or rays_d.requires_grad))):
        use_fused = False
    if not use_fused:
        return _torch_route(space, rays_o, rays_d, t_min, radius_scale_max, include_inf_distance, perturb, mode, interval_type, table)
    radii, step_size, log_min, log_max = table
    radii = radii.float()                                      # arange of Python floats is float32 already: no copy
    noise = torch.rand([rays_o.shape[0], radii.shape[0]], device=rays_o.device, dtype=torch.float32) if perturb else None
    out = _nerfpp_march.nerfpp_march(
        rays_o.detach().contiguous(), rays_d.detach().contiguous(), t_min.detach().contiguous(), aabb.detach().contiguous(), radii, noise,
        step=step_size, last_radius=1.0e10 if include_inf_distance else radius_scale_max, sample_mode=mode, interval_type=interval_type,
        log_min=0.0 if log_min is None else log_min, log_max=1.0 if log_max is None else log_max)
    if out is None:
        return nerfpp_raymarch_ret(None, None, None, None, None, None)
    return nerfpp_raymarch_ret(out['ridx_hit'], out['samples'], out['depth_samples'], out['deltas'], out['ridx'], out['pack_infos'])
