"""Rendering mixin of a time-varying NeuS model -- counterpart of ``NeusRendererMixinDynamic``
(nr3d_lib/models/fields_dynamic/neus/renderer_mixin.py:75-440)."""
from typing import Dict, List

import torch

from nr3d_lib_amd.graphics.neus.neus_ray_query import (neus_ray_query_coarse_multi_upsample, neus_ray_query_march_occ_multi_upsample,
                                                        neus_ray_query_march_occ_multi_upsample_compressed,
                                                        neus_ray_query_sphere_trace)
from nr3d_lib_amd.graphics.neus.neus_render import composite_volume_buffer

__all__ = ['NeusRendererMixinDynamic']

_QUERY_MODES = dict(march_occ_multi_upsample=neus_ray_query_march_occ_multi_upsample,
                    march_occ_multi_upsample_compressed=neus_ray_query_march_occ_multi_upsample_compressed,
                    coarse_multi_upsample=neus_ray_query_coarse_multi_upsample,
                    sphere_trace=neus_ray_query_sphere_trace)
_NOT_IMPLEMENTED = ('march_occ_multi_upsample_compressed_strategy', 'march_occ')      # as in the reference's mixin


def _cfg(config, key, default=None):
    return config.get(key, default) if isinstance(config, dict) else getattr(config, key, default)


class NeusRendererMixinDynamic:
    """Put in front of a network class: ``class Model(NeusRendererMixinDynamic, Net)``.  The constructor takes the reference's renderer
    keywords and hands every other keyword to the next class (``super().__init__(**net_kwargs)``).  The network provides ``space`` (an
    ``AABBDynamicSpace``), ``forward_sdf(x, ts=)`` -> dict with 'sdf', ``forward_sdf_nablas(x, ts=)``, ``query_sdf(x, ts=)`` -> sdf,
    ``forward(x, ts=, nablas_has_grad=, with_rgb=, with_normal=, ...)`` and ``forward_inv_s()``.  ``accel``: a dynamic acceleration
    structure over ``space`` (``OccGridAccelDynamic``), given ready-made or left None -- the reference builds it from ``accel_cfg``
    through its ``get_accel`` registry, which this library does not have; ``accel_cfg`` is stored.

    ``forward_sdf`` / ``forward_sdf_nablas`` hand their samples to ``accel.collect_samples(x, ts=, val=sdf)`` while training.
    ``ray_query`` dispatches ``config.query_mode`` to the drivers of ``graphics.neus.neus_ray_query``; 'march_occ' and
    'march_occ_multi_upsample_compressed_strategy' raise NotImplementedError as in the reference.

    LEFT OUT: the sample annealer (``sample_anneal_cfg`` is stored), ``training_after_per_step`` / ``shrink``."""

    use_view_dirs: bool = False
    use_nablas: bool = False
    use_h_appear: bool = False
    use_ts: bool = True             # the ray queries pass ray_tested['rays_ts'] of every sample's ray as `ts`
    use_pix: bool = False
    use_fidx: bool = False
    use_bidx: bool = False
    fwd_sdf_use_pix: bool = False
    fwd_sdf_use_h_appear: bool = False
    fwd_sdf_use_view_dirs: bool = False

    def __init__(self, ray_query_cfg: dict = dict(), accel_cfg: dict = None, sample_anneal_cfg: dict = None,
                 shrink_milestones: List[int] = [], accel=None, **net_kwargs) -> None:
        mro = type(self).mro()
        assert mro[mro.index(NeusRendererMixinDynamic) + 1] is not object, \
            "NeusRendererMixinDynamic comes before the network class when inheriting and is not instantiated on its own"
        super().__init__(**net_kwargs)
        self.ray_query_cfg = ray_query_cfg
        self.accel_cfg = accel_cfg
        self.sample_anneal_cfg = sample_anneal_cfg
        self.shrink_milestones = shrink_milestones
        self.accel = accel
        self.upsample_s_divisor = 1.0

    def _sample_pts(self, x, ts):
        ret = self.forward_sdf_nablas(x, ts=ts, skip_accel=True)    # too few samples to be worth collecting
        ret = {k: v.to(x.dtype) for k, v in ret.items()}
        ret['net_x'] = x                                            # in the network's normalised space, not in world space
        return ret

    def sample_pts_uniform(self, num_samples: int):
        return self._sample_pts(*self.space.sample_pts_uniform(num_samples))

    def sample_pts_in_occupied(self, num_samples: int):
        assert self.accel is not None, "Requires self.accel not to be None"
        return self._sample_pts(*self.accel.sample_pts_in_occupied(num_samples))

    def forward_sdf(self, x: torch.Tensor, ts: torch.Tensor, skip_accel=False, **kwargs):
        ret = super().forward_sdf(x, ts=ts, **kwargs)
        if self.training and (not skip_accel) and (self.accel is not None):
            self.accel.collect_samples(x, ts=ts, val=ret['sdf'].data)
        return ret

    def forward_sdf_nablas(self, x: torch.Tensor, ts: torch.Tensor, skip_accel=False, **kwargs):
        ret = super().forward_sdf_nablas(x, ts=ts, **kwargs)
        if self.training and (not skip_accel) and (self.accel is not None):
            self.accel.collect_samples(x, ts=ts, val=ret['sdf'].data)
        return ret

    @torch.no_grad()
    def query_sdf(self, x: torch.Tensor, ts: torch.Tensor, **kwargs):
        return super().query_sdf(x, ts=ts, **kwargs)

    def training_initialize(self, config=dict(), logger=None, log_prefix: str = None, skip_accel=False) -> bool:
        parent = getattr(super(), 'training_initialize', None)
        updated = bool(parent(config, logger=logger, log_prefix=log_prefix)) if parent is not None else False
        if (not skip_accel) and (self.accel is not None):
            self.accel.init(self.query_sdf, logger=logger)
        return updated

    def training_before_per_step(self, cur_it: int, logger=None, skip_accel=False):
        self.it = cur_it
        parent = getattr(super(), 'training_before_per_step', None)
        if parent is not None:
            parent(cur_it, logger=logger)
        if (not skip_accel) and (self.accel is not None):
            self.upsample_s_divisor = 2 ** self.accel.training_granularity
            if self.training:
                self.accel.step(cur_it, self.query_sdf, logger)

    def ray_test(self, rays_o: torch.Tensor, rays_d: torch.Tensor, near=None, far=None, **extra_ray_data: Dict[str, torch.Tensor]):
        assert (rays_o.dim() == 2) and (rays_d.dim() == 2), "Expect `rays_o` and `rays_d` to be of shape [N, 3]"
        for k, v in extra_ray_data.items():
            if isinstance(v, torch.Tensor):
                assert v.shape[0] == rays_o.shape[0], \
                    f"Expect `{k}` has the same shape prefix with rays_o {rays_o.shape[0]}, but got {v.shape[0]}"
        return self.space.ray_test(rays_o, rays_d, near=near, far=far, return_rays=True, **extra_ray_data)

    def ray_query(self, ray_input: Dict[str, torch.Tensor] = None, ray_tested: Dict[str, torch.Tensor] = None, config=dict(),
                  return_buffer=False, return_details=False, render_per_obj_individual=False) -> dict:
        """``config`` (attributes or dict keys): query_mode, with_rgb, with_normal, perturb, query_param (the keywords of the driver),
        optionally forward_inv_s, depth_use_normalized_vw, with_near_sdf.  -> dict with 'volume_buffer' (return_buffer), 'details'
        (return_details) and 'rendered' (render_per_obj_individual: depth_volume, mask_volume [num_total_rays], rgb_volume /
        normals_volume [num_total_rays, 3]; rays that hit nothing keep zeros)."""
        if ray_tested is None:
            assert ray_input is not None
            ray_tested = self.ray_test(**ray_input)
        query_mode, with_rgb, with_normal = _cfg(config, 'query_mode'), bool(_cfg(config, 'with_rgb')), bool(_cfg(config, 'with_normal'))
        forward_inv_s = _cfg(config, 'forward_inv_s', None)
        if forward_inv_s is None:
            forward_inv_s = self.forward_inv_s()

        raw_ret = dict()
        if return_buffer:
            raw_ret['volume_buffer'] = dict(type='empty', rays_inds_hit=[])
        if return_details:
            details = raw_ret['details'] = {}
            details['inv_s'] = forward_inv_s.item() if isinstance(forward_inv_s, torch.Tensor) else forward_inv_s
            details['s'] = 1. / details['inv_s']
            if (self.accel is not None) and hasattr(self.accel, 'debug_stats'):
                details['accel'] = self.accel.debug_stats()
        if render_per_obj_individual:
            prefix_rays, device = ray_input['rays_o'].shape[:-1], ray_input['rays_o'].device
            raw_ret['rendered'] = rendered = composite_volume_buffer(dict(type='empty'), prefix_rays.numel(), with_rgb=with_rgb,
                                                                     with_normal=with_normal, device=device)
            for k, v in rendered.items():
                rendered[k] = v.view(*prefix_rays, *v.shape[1:])
        if ray_tested['num_rays'] == 0:
            return raw_ret

        if query_mode in _NOT_IMPLEMENTED:
            raise NotImplementedError
        if query_mode not in _QUERY_MODES:
            raise RuntimeError(f"Invalid query_mode={query_mode}")
        # (the sphere tracer samples no volume: no opacity scale, no up-sampling)
        extra = {} if query_mode == 'sphere_trace' else dict(forward_inv_s=forward_inv_s, upsample_s_divisor=self.upsample_s_divisor)
        volume_buffer, query_details = _QUERY_MODES[query_mode](
            self, ray_tested, with_rgb=with_rgb, with_normal=with_normal, perturb=_cfg(config, 'perturb', False), **extra,
            **(_cfg(config, 'query_param', None) or {}))

        if return_buffer:
            raw_ret['volume_buffer'] = volume_buffer
        if return_details:
            details.update(query_details)
            if _cfg(config, 'with_near_sdf', False):
                kw = dict(x=torch.addcmul(ray_tested['rays_o'], ray_tested['rays_d'], ray_tested['near'].unsqueeze(-1)))
                if self.use_ts:
                    kw['ts'] = ray_tested['rays_ts']
                if self.use_fidx:
                    kw['fidx'] = ray_tested['rays_fidx']
                details['near_sdf'] = self.forward_sdf(**kw)['sdf']
        if render_per_obj_individual and volume_buffer['type'] != 'empty':
            out = composite_volume_buffer(volume_buffer, prefix_rays.numel(), with_rgb=with_rgb, with_normal=with_normal,
                                          training=bool(getattr(self, 'training', False)),
                                          depth_use_normalized_vw=_cfg(config, 'depth_use_normalized_vw', True), device=device)
            for k, v in out.items():
                rendered[k] = v.view(*prefix_rays, *v.shape[1:])
        return raw_ret
