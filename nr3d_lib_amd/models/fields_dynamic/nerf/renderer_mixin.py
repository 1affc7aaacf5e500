"""Rendering mixin of a time-varying NeRF -- counterpart of ``NerfRendererMixinDynamic``
(nr3d_lib/models/fields_dynamic/nerf/renderer_mixin.py:23-326), plus the decomposed static / dynamic render that the reference keeps
inside its EmerNeRF model (fields_dynamic/nerf/emernerf.py:806-938; here ``graphics.nerf.nerf_dynamic_render``)."""
from typing import Dict

import torch

from nr3d_lib_amd.graphics.nerf.nerf_dynamic_render import composite_static_dynamic
from nr3d_lib_amd.graphics.nerf.nerf_ray_query import (nerf_ray_query_march_occ,
                                                        nerf_ray_query_march_occ_multi_upsample_compressed)
from nr3d_lib_amd.graphics.neus.neus_render import composite_volume_buffer

__all__ = ['NerfRendererMixinDynamic']

_QUERY_MODES = dict(march_occ=nerf_ray_query_march_occ,
                    march_occ_multi_upsample_compressed=nerf_ray_query_march_occ_multi_upsample_compressed)


def _cfg(config, key, default=None):
    return config.get(key, default) if isinstance(config, dict) else getattr(config, key, default)


class NerfRendererMixinDynamic:
    """Put in front of a network class: ``class Model(NerfRendererMixinDynamic, Net)``.  The constructor takes the reference's renderer
    keywords and hands every other keyword to the next class (``super().__init__(**net_kwargs)``).  The network provides ``space`` (an
    ``AABBDynamicSpace``), ``forward(x, ts=, ...)`` -> dict with 'sigma' (and 'rgb'), ``forward_density(x, ts=)`` -> dict with 'sigma' and
    ``query_density(x, ts=)`` -> sigma.  ``accel``: a dynamic acceleration structure over ``space`` (``OccGridAccelDynamic``,
    ``OccGridAccelStaticAndDynamic``), given ready-made or left None -- the reference builds it from ``accel_cfg`` through its
    ``get_accel`` registry, which this library does not have; ``accel_cfg`` is stored.

    ``forward`` / ``forward_density`` hand their samples to ``accel.collect_samples`` while training.  The combined accel wants a static
    and a dynamic value: the network's 'sigma_static' / 'sigma_dynamic' where it returns them, else 'sigma' for both.
    ``ray_query`` dispatches ``config.query_mode`` ('march_occ', 'march_occ_multi_upsample_compressed'); with
    ``config.with_static_dynamic`` the buffer gets ``opacity_alpha_static`` / ``_dynamic`` and ``rendered`` the decomposed keys of
    ``composite_static_dynamic`` (flows with ``config.with_flow``)."""

    use_view_dirs: bool = False
    use_nablas: bool = False
    use_h_appear: bool = False
    use_ts: bool = True             # the ray queries pass ray_tested['rays_ts'] of every sample's ray as `ts`
    use_pix: bool = False
    use_fidx: bool = False
    use_bidx: bool = False
    fwd_density_use_pix: bool = False
    fwd_density_use_h_appear: bool = False
    fwd_density_use_view_dirs: bool = False

    def __init__(self, ray_query_cfg: dict = dict(), accel_cfg: dict = None, accel=None, **net_kwargs) -> None:
        mro = type(self).mro()
        assert mro[mro.index(NerfRendererMixinDynamic) + 1] is not object, \
            "NerfRendererMixinDynamic comes before the network class when inheriting and is not instantiated on its own"
        super().__init__(**net_kwargs)
        self.ray_query_cfg = ray_query_cfg
        self.accel_cfg = accel_cfg
        self.accel = accel

    def _sample_pts(self, x, ts):
        ret = self.forward_density(x, ts=ts, skip_accel=True)       # too few samples to be worth collecting
        ret = {k: v.to(x.dtype) for k, v in ret.items()}
        ret['net_x'] = x                                            # in the network's normalised space, not in world space
        return ret

    def sample_pts_uniform(self, num_samples: int):
        return self._sample_pts(*self.space.sample_pts_uniform(num_samples))

    def sample_pts_in_occupied(self, num_samples: int):
        assert self.accel is not None, "Requires self.accel not to be None"
        return self._sample_pts(*self.accel.sample_pts_in_occupied(num_samples))

    def _collect(self, x, ts, ret):
        if hasattr(self.accel, 'occ_static'):
            sigma = ret['sigma'].data
            self.accel.collect_samples(x, ts=ts, val_static=ret['sigma_static'].data if 'sigma_static' in ret else sigma,
                                       val_dynamic=ret['sigma_dynamic'].data if 'sigma_dynamic' in ret else sigma)
        else:
            self.accel.collect_samples(x, ts=ts, val=ret['sigma'].data)

    def forward_density(self, x: torch.Tensor, ts: torch.Tensor, skip_accel=False, **kwargs):
        ret = super().forward_density(x, ts=ts, **kwargs)
        if self.training and (not skip_accel) and (self.accel is not None):
            self._collect(x, ts, ret)
        return ret

    @torch.no_grad()
    def query_density(self, x: torch.Tensor, ts: torch.Tensor, **kwargs):
        return super().query_density(x, ts=ts, **kwargs)

    def forward(self, x: torch.Tensor, ts: torch.Tensor, skip_accel=False, **kwargs):
        ret = super().forward(x, ts=ts, **kwargs)
        if self.training and (not skip_accel) and (self.accel is not None):
            self._collect(x, ts, ret)
        return ret

    def _accel_fns(self):
        """what ``accel.init`` / ``accel.step`` take: one density query, or (static, dynamic) for the combined accel -- the network's
        ``query_density_static(x)`` / ``query_density_dynamic(x, ts=)``"""
        if hasattr(self.accel, 'occ_static'):
            assert hasattr(self, 'query_density_static') and hasattr(self, 'query_density_dynamic'), \
                "a static + dynamic accel needs the network's query_density_static(x) and query_density_dynamic(x, ts=)"
            return self.query_density_static, self.query_density_dynamic
        return (self.query_density,)

    def training_initialize(self, config=dict(), logger=None, log_prefix: str = None, skip_accel=False) -> bool:
        parent = getattr(super(), 'training_initialize', None)
        updated = bool(parent(config, logger=logger, log_prefix=log_prefix)) if parent is not None else False
        if (not skip_accel) and (self.accel is not None):
            self.accel.init(*self._accel_fns(), logger=logger)
        return updated

    def training_before_per_step(self, cur_it: int, logger=None, skip_accel=False):
        self.it = cur_it
        parent = getattr(super(), 'training_before_per_step', None)
        if parent is not None:
            parent(cur_it, logger=logger)
        if self.training and (not skip_accel) and (self.accel is not None):
            self.accel.step(cur_it, *self._accel_fns(), logger=logger)

    def ray_test(self, rays_o: torch.Tensor, rays_d: torch.Tensor, near=None, far=None, **extra_ray_data: Dict[str, torch.Tensor]):
        """slab test against the space's box -> num_rays, rays_inds, rays_o, rays_d (normalised), near, far and the extras of the hit
        rays (``rays_ts`` among them)"""
        assert (rays_o.dim() == 2) and (rays_d.dim() == 2), "Expect `rays_o` and `rays_d` to be of shape [N, 3]"
        for k, v in extra_ray_data.items():
            if isinstance(v, torch.Tensor):
                assert v.shape[0] == rays_o.shape[0], \
                    f"Expect `{k}` has the same shape prefix with rays_o {rays_o.shape[0]}, but got {v.shape[0]}"
        return self.space.ray_test(rays_o, rays_d, near=near, far=far, return_rays=True, **extra_ray_data)

    def ray_query(self, ray_input: Dict[str, torch.Tensor] = None, ray_tested: Dict[str, torch.Tensor] = None, config=dict(),
                  return_buffer=False, return_details=False, render_per_obj_individual=False) -> dict:
        """``config`` (attributes or dict keys): query_mode, with_rgb, with_normal, perturb, query_param (the keywords of the driver),
        optionally depth_use_normalized_vw, with_static_dynamic, with_flow, forward_params.  -> dict with 'volume_buffer'
        (return_buffer), 'details' (return_details) and 'rendered' (render_per_obj_individual: depth_volume, mask_volume
        [num_total_rays], rgb_volume / normals_volume [num_total_rays, 3], and the decomposed keys; rays that hit nothing keep zeros)."""
        if ray_tested is None:
            assert ray_input is not None
            ray_tested = self.ray_test(**ray_input)
        query_mode, with_rgb, with_normal = _cfg(config, 'query_mode'), bool(_cfg(config, 'with_rgb')), bool(_cfg(config, 'with_normal'))
        with_sd, with_flow = bool(_cfg(config, 'with_static_dynamic', False)), bool(_cfg(config, 'with_flow', False))
        training = bool(getattr(self, 'training', False))
        norm_vw = _cfg(config, 'depth_use_normalized_vw', True)

        raw_ret = dict()
        if return_buffer:
            raw_ret['volume_buffer'] = dict(type='empty', rays_inds_hit=[])
        if return_details:
            details = raw_ret['details'] = {}
            if (self.accel is not None) and hasattr(self.accel, 'debug_stats'):
                details['accel'] = self.accel.debug_stats()

        def render(volume_buffer):
            has_normal = with_normal and (volume_buffer['type'] == 'empty' or 'nablas' in volume_buffer)
            out = composite_volume_buffer(volume_buffer, n_total, with_rgb=with_rgb, with_normal=has_normal, training=training,
                                          depth_use_normalized_vw=norm_vw, device=device)
            if with_normal and not has_normal:
                out['normals_volume'] = torch.zeros(n_total, 3, device=device)
            if with_sd:
                out.update(composite_static_dynamic(volume_buffer, n_total, with_rgb=with_rgb, with_normal=with_normal,
                                                    with_flow=with_flow, training=training, depth_use_normalized_vw=norm_vw,
                                                    device=device))
            return {k: v.view(*prefix_rays, *v.shape[1:]) for k, v in out.items()}

        if render_per_obj_individual:
            prefix_rays, device = ray_input['rays_o'].shape[:-1], ray_input['rays_o'].device
            n_total = prefix_rays.numel()
            raw_ret['rendered'] = render(dict(type='empty'))
        if ray_tested['num_rays'] == 0:
            return raw_ret

        if query_mode not in _QUERY_MODES:
            raise RuntimeError(f"Invalid query_mode={query_mode}")
        extra = {} if _cfg(config, 'forward_params', None) is None else dict(forward_params=_cfg(config, 'forward_params'))
        volume_buffer, query_details = _QUERY_MODES[query_mode](self, ray_tested, with_rgb=with_rgb, perturb=_cfg(config, 'perturb', False),
                                                                **extra, **(_cfg(config, 'query_param', None) or {}))
        if with_sd and volume_buffer['type'] != 'empty':
            from nr3d_lib_amd.graphics.nerf.nerf_dynamic_render import _side_alphas
            _side_alphas(volume_buffer)

        if return_buffer:
            raw_ret['volume_buffer'] = volume_buffer
        if return_details:
            details.update(query_details)
        if render_per_obj_individual and volume_buffer['type'] != 'empty':
            raw_ret['rendered'] = render(volume_buffer)
        return raw_ret
