"""The ray query of the distant-view NeRF++ model: shell march -> (prune) -> query -> volume buffer.

Counterpart of ``NeRFRendererMixinDistant._ray_query_march`` and ``.ray_query`` (nr3d_lib/models/fields_distant/nerf/
renderer_mixin.py:290-380, :383-540) as functions of a duck-typed model:
  ``model.space`` (the close-range AABBSpace), ``model.radius_scale_min`` / ``radius_scale_max`` / ``include_inf_distance`` feed
  ``nerfpp_raymarch`` (graphics/raymarch/nerfpp_raymarch.py: HIP kernels under FUSED_NERFPP_MARCH, the reference's chain otherwise);
  ``model.forward_density(x)['sigma']`` on the 4-D samples prunes them under no_grad; ``model.forward(x=, v=, h_appear=)`` or
  ``model.forward_density(x)`` is the differentiable query; opacity = ``sigma_delta_to_alpha(sigma, deltas)``.
The pruning is ``packed_volume_render_compression`` + index gathers: the library's gathering compaction moves 3-column rows only.
The rendered dict of ``nerf_distant_ray_query`` comes from ``composite_packed_volume_buffer`` (one launch, ``packed_composite``)."""
from operator import itemgetter
from typing import Dict, Tuple

import torch

from nr3d_lib_amd.graphics.nerf.nerf_ray_query import composite_packed_volume_buffer
from nr3d_lib_amd.graphics.nerf.nerf_utils import sigma_delta_to_alpha
from nr3d_lib_amd.graphics.pack_ops import packed_volume_render_compression
from nr3d_lib_amd.graphics.raymarch.nerfpp_raymarch import nerfpp_raymarch, nerfpp_raymarch_ret

__all__ = ['nerf_distant_ray_query_march', 'nerf_distant_ray_query']


def _cfg(config, key, default=None):
    return config.get(key, default) if isinstance(config, dict) else getattr(config, key, default)


def nerf_distant_ray_query_march(model, ray_tested: Dict[str, torch.Tensor], *, with_rgb=True, with_normal=False, perturb=False,
                                 march_cfg={}, compression=True, bypass_sigma_fn=None, bypass_alpha_fn=None) -> Tuple[dict, dict]:
    """-> (volume_buffer, details).  ``ray_tested``: num_rays, rays_o / rays_d [num_rays, 3] in the model's object space, near (shells
    closer than it are dropped), far, rays_inds, optionally rays_h_appear.  ``march_cfg``: max_steps, sample_mode, interval_type (and
    ``fused``) of ``nerfpp_raymarch``.  ``bypass_sigma_fn`` / ``bypass_alpha_fn`` receive the nerfpp_raymarch_ret and replace the pruning
    query.  volume_buffer: type 'packed', rays_inds_hit, pack_infos_hit, t, [rgb,] sigma, opacity_alpha -- or dict(type='empty',
    rays_inds_hit=[]); details: 'march.num_per_ray', 'render.num_per_ray' and, with compression, 'render.num_per_ray0'."""
    empty_volume_buffer = dict(type='empty', rays_inds_hit=[])
    if ray_tested['num_rays'] == 0:
        return empty_volume_buffer, {}
    rays_o, rays_d, near, far, rays_inds = itemgetter("rays_o", "rays_d", "near", "far", "rays_inds")(ray_tested)
    assert (rays_o.dim() == 2) and (rays_d.dim() == 2)
    dtype = rays_o.dtype

    ret = nerfpp_raymarch(model.space, rays_o, rays_d, near, far, radius_scale_min=model.radius_scale_min,
                          radius_scale_max=model.radius_scale_max, include_inf_distance=model.include_inf_distance, perturb=perturb,
                          **march_cfg)
    if ret.ridx_hit is None:
        return empty_volume_buffer, {}

    if compression:
        with torch.no_grad():
            assert int(bypass_sigma_fn is not None) + int(bypass_alpha_fn is not None) <= 1, \
                "Please pass at most one of bypass_sigma_fn or bypass_alpha_fn"
            if bypass_alpha_fn is not None:
                alphas = bypass_alpha_fn(ret)
            else:
                sigmas = bypass_sigma_fn(ret) if bypass_sigma_fn is not None else model.forward_density(ret.samples)['sigma']
                alphas = sigma_delta_to_alpha(sigmas.view(-1), ret.deltas.view(-1))
        old_pack_infos = ret.pack_infos.clone()
        nidx_useful, pack_infos_hit_useful, pidx_useful = packed_volume_render_compression(alphas.view(-1), ret.pack_infos)
        if nidx_useful.numel() == 0:
            return empty_volume_buffer, {}
        ret = nerfpp_raymarch_ret(ret.ridx_hit[nidx_useful], ret.samples[pidx_useful], ret.depth_samples[pidx_useful],
                                  ret.deltas[pidx_useful], ret.ridx[pidx_useful], pack_infos_hit_useful)

    volume_buffer = dict(type='packed', rays_inds_hit=rays_inds[ret.ridx_hit], pack_infos_hit=ret.pack_infos, t=ret.depth_samples.to(dtype))
    if compression:
        details = {'march.num_per_ray': old_pack_infos[:, 1], 'render.num_per_ray0': old_pack_infos[:, 1],
                   'render.num_per_ray': ret.pack_infos[:, 1]}
    else:
        details = {'march.num_per_ray': ret.pack_infos[:, 1], 'render.num_per_ray': ret.pack_infos[:, 1]}

    if with_rgb:
        # the scale rays_d carries is a length scale along the ray, not part of the view direction
        view_dirs = rays_d / rays_d.detach().norm(dim=-1).clamp_min(1.0e-10).unsqueeze(-1)
        h_appear = ray_tested['rays_h_appear'][ret.ridx] if ray_tested.get('rays_h_appear', None) is not None else None
        net_out = model.forward(x=ret.samples, v=view_dirs[ret.ridx], h_appear=h_appear)
        volume_buffer["rgb"] = net_out["rgb"].to(dtype)
    else:
        net_out = model.forward_density(ret.samples)
    volume_buffer["sigma"] = net_out["sigma"].to(dtype)
    volume_buffer["opacity_alpha"] = sigma_delta_to_alpha(net_out["sigma"].view(-1), ret.deltas.view(-1)).view(net_out["sigma"].shape).to(dtype)
    return volume_buffer, details


def nerf_distant_ray_query(model, ray_input: Dict[str, torch.Tensor] = None, ray_tested: Dict[str, torch.Tensor] = None,
                           config=dict(), return_buffer=False, return_details=False, render_per_obj_individual=False) -> dict:
    """The reference's ``ray_query`` (``config.query_mode == 'march'`` only): ``config`` has query_mode, with_rgb, with_normal, perturb,
    query_param (the keywords of ``nerf_distant_ray_query_march``) and optionally depth_use_normalized_vw -- as attributes or as dict
    keys.  -> dict with 'volume_buffer' (return_buffer), 'details' (return_details) and 'rendered' (render_per_obj_individual:
    mask_volume, depth_volume [num_total_rays], rgb_volume [num_total_rays, 3] with with_rgb; rays that were not hit keep zeros;
    ``ray_input['rays_o']`` gives the number of rays).  Without ``ray_tested``, ``model.ray_test(**ray_input)`` provides it."""
    if ray_tested is None:
        assert ray_input is not None
        ray_tested = model.ray_test(**ray_input)
    query_mode, with_rgb, with_normal = _cfg(config, 'query_mode'), _cfg(config, 'with_rgb'), _cfg(config, 'with_normal', False)

    raw_ret = {}
    if return_buffer:
        raw_ret['volume_buffer'] = dict(type='empty', rays_inds_hit=[])
    if return_details:
        raw_ret['details'] = details = {}
        accel = getattr(model, 'accel', None)
        if (accel is not None) and hasattr(accel, 'debug_stats'):
            details['accel'] = accel.debug_stats()
    if render_per_obj_individual:
        prefix = ray_input["rays_o"][..., 0]
        raw_ret['rendered'] = rendered = {"depth_volume": torch.zeros_like(prefix), "mask_volume": torch.zeros_like(prefix)}
        if with_rgb:
            rendered['rgb_volume'] = torch.zeros_like(ray_input["rays_o"])
        if with_normal:
            rendered['normals_volume'] = torch.zeros_like(ray_input["rays_o"])
    if ray_tested['num_rays'] == 0:
        return raw_ret

    if query_mode == 'march':
        volume_buffer, query_details = nerf_distant_ray_query_march(
            model, ray_tested, with_rgb=with_rgb, perturb=_cfg(config, 'perturb', False), **(_cfg(config, 'query_param', None) or {}))
    else:
        raise RuntimeError(f"Invalid query_mode={query_mode}")

    if return_buffer:
        raw_ret['volume_buffer'] = volume_buffer
    if return_details:
        details.update(query_details)
    if render_per_obj_individual and volume_buffer['type'] != 'empty':
        out = composite_packed_volume_buffer(volume_buffer, prefix.numel(), with_rgb=bool(with_rgb),
                                             depth_use_normalized_vw=_cfg(config, 'depth_use_normalized_vw', True),
                                             device=prefix.device, dtype=prefix.dtype)
        rendered['mask_volume'] = out['mask_volume'].view(prefix.shape)
        rendered['depth_volume'] = out['depth_volume'].view(prefix.shape)
        if with_rgb:
            rendered['rgb_volume'] = out['rgb_volume'].view(ray_input["rays_o"].shape)
    return raw_ret
