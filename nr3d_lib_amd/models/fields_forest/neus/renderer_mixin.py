"""Rendering mixin of the forest NeuS model -- counterpart of ``NeuSRendererMixinForest``
(nr3d_lib/models/fields_forest/neus/renderer_mixin.py:31-887)."""
from typing import Dict

import torch

from nr3d_lib_amd.graphics.neus.neus_forest_ray_query import (neus_forest_ray_query_coarse_multi_upsample,
                                                              neus_forest_ray_query_march_occ_multi_upsample,
                                                              neus_forest_ray_query_march_occ_multi_upsample_compressed)
from nr3d_lib_amd.graphics.neus.neus_render import composite_volume_buffer

__all__ = ['NeuSRendererMixinForest']

_QUERY_MODES = dict(inblock_coarse_multi_upsample=neus_forest_ray_query_coarse_multi_upsample,
                    inblock_march_occ_multi_upsample=neus_forest_ray_query_march_occ_multi_upsample,
                    inblock_march_occ_multi_upsample_compressed=neus_forest_ray_query_march_occ_multi_upsample_compressed)


def _cfg(config, key, default=None):
    return config.get(key, default) if isinstance(config, dict) else getattr(config, key, default)


class NeuSRendererMixinForest:
    """Put in front of a network class: ``class Model(NeuSRendererMixinForest, Net)``.  The constructor takes the reference's renderer
    keywords and hands every other keyword to the next class (``super().__init__(**net_kwargs)``).  The network provides ``space`` (a
    populated ForestBlockSpace), ``forward_sdf(x, block_inds, block_offsets, input_normalized=)``, ``forward_sdf_nablas`` likewise,
    ``forward(x, v, block_inds, h_appear=, nablas_has_grad=, with_rgb=, with_normal=)``, ``forward_inv_s()`` and ``use_view_dirs``.
    ``accel``: an acceleration structure over ``space`` (``OccGridAccelForest``), given ready-made or left None -- the reference builds
    it from ``accel_cfg`` through its ``get_accel`` registry, which this library does not have; ``accel_cfg`` is stored.

    ``ray_query`` dispatches ``config.query_mode`` to the three drivers of ``graphics.neus.neus_forest_ray_query``.

    LEFT OUT: the training hooks of the reference's class (``populate``, ``training_initialize``, ``training_before_per_step``,
    ``training_after_per_step``, ``query_sdf``); ``upsample_s_divisor`` therefore stays 1 unless the owner sets it."""

    def __init__(self, ray_query_cfg: dict = dict(), accel_cfg: dict = None, accel=None, **net_kwargs) -> None:
        mro = type(self).mro()
        assert mro[mro.index(NeuSRendererMixinForest) + 1] is not object, \
            "NeuSRendererMixinForest comes before the network class when inheriting and is not instantiated on its own"
        super().__init__(**net_kwargs)
        self.ray_query_cfg = ray_query_cfg
        self.accel_cfg = accel_cfg
        self.accel = accel
        self.upsample_s_divisor = 1.0

    def _sample_pts(self, block_x, blidx):
        ret = self.forward_sdf_nablas(block_x, blidx, input_normalized=True, skip_accel=True)
        ret = {k: v.to(block_x.dtype) for k, v in ret.items()}
        ret['net_x'] = block_x                      # in the blocks' normalised coordinates, not in world space
        if 'nablas' in ret:
            ret['nablas_norm'] = ret['nablas'].norm(dim=-1)
        return ret

    def sample_pts_uniform(self, num_samples: int):
        return self._sample_pts(*self.space.sample_pts_uniform(num_samples))

    def sample_pts_in_occupied(self, num_samples: int):
        assert self.accel is not None, "Requires self.accel not to be None"
        return self._sample_pts(*self.accel.sample_pts_in_occupied(num_samples))

    def forward_sdf(self, x: torch.Tensor, block_inds: torch.Tensor = None, block_offsets: torch.Tensor = None, skip_accel=False,
                    input_normalized=False, **kwargs):
        """the network's ``forward_sdf``; the samples go to the acceleration structure (which keeps them while training)"""
        ret = super().forward_sdf(x, block_inds, block_offsets, input_normalized=input_normalized, **kwargs)
        if (not skip_accel) and (self.accel is not None):
            self.accel.collect_samples(x, block_inds, ret['sdf'].data, normalized=input_normalized)
        return ret

    def forward_sdf_nablas(self, x: torch.Tensor, block_inds: torch.Tensor = None, block_offsets: torch.Tensor = None,
                           skip_accel=False, input_normalized=False, **kwargs):
        ret = super().forward_sdf_nablas(x, block_inds, block_offsets, input_normalized=input_normalized, **kwargs)
        if (not skip_accel) and (self.accel is not None):
            self.accel.collect_samples(x, block_inds, ret['sdf'].data, normalized=input_normalized)
        return ret

    def ray_test(self, rays_o: torch.Tensor, rays_d: torch.Tensor, near=None, far=None, return_rays=True, **extra_ray_data):
        assert (rays_o.dim() == 2) and (rays_d.dim() == 2), "Expect rays_o and rays_d to be of shape [N, 3]"
        return self.space.ray_test(rays_o, rays_d, near=near, far=far, return_rays=return_rays, **extra_ray_data)

    def ray_query(self, ray_input: Dict[str, torch.Tensor] = None, ray_tested: Dict[str, torch.Tensor] = None, config=dict(),
                  return_buffer=False, return_details=False, render_per_obj_individual=False):
        """``config`` (attributes or dict keys): query_mode, with_rgb, with_normal, perturb, query_param (the keywords of the driver),
        optionally forward_inv_s, depth_use_normalized_vw, with_near_sdf.  -> dict with 'volume_buffer' (return_buffer), 'details'
        (return_details) and 'rendered' (render_per_obj_individual: depth_volume, mask_volume [num_total_rays], rgb_volume /
        normals_volume [num_total_rays, 3]; rays that hit nothing keep zeros; ``ray_input['rays_o']`` gives the number of rays).
        Without ``ray_tested``, ``self.ray_test(**ray_input)`` provides it."""
        if ray_tested is None:
            assert ray_input is not None
            ray_tested = self.ray_test(**ray_input, return_rays=True)
        query_mode, with_rgb, with_normal = _cfg(config, 'query_mode'), _cfg(config, 'with_rgb'), _cfg(config, 'with_normal')
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
            raw_ret['rendered'] = rendered = composite_volume_buffer(
                dict(type='empty'), prefix_rays.numel(), with_rgb=bool(with_rgb), with_normal=bool(with_normal), device=device)
            for k, v in rendered.items():
                rendered[k] = v.view(*prefix_rays, *v.shape[1:])
        if ray_tested['num_rays'] == 0:
            return raw_ret

        if query_mode not in _QUERY_MODES:
            raise RuntimeError(f"Invalid query_mode={query_mode}")
        volume_buffer, query_details = _QUERY_MODES[query_mode](
            self, ray_tested, with_rgb=with_rgb, with_normal=with_normal, perturb=_cfg(config, 'perturb', False),
            forward_inv_s=forward_inv_s, **(_cfg(config, 'query_param', None) or {}))

        if return_buffer:
            raw_ret['volume_buffer'] = volume_buffer
        if return_details:
            details.update(query_details)
            if _cfg(config, 'with_near_sdf', False):
                x_near = torch.addcmul(ray_tested['rays_o'], ray_tested['rays_d'], ray_tested['near'].unsqueeze(-1))
                details['near_sdf'] = self.forward_sdf(x_near, input_normalized=False)['sdf']
        if render_per_obj_individual and volume_buffer['type'] != 'empty':
            out = composite_volume_buffer(volume_buffer, prefix_rays.numel(), with_rgb=bool(with_rgb), with_normal=bool(with_normal),
                                          training=bool(getattr(self, 'training', False)),
                                          depth_use_normalized_vw=_cfg(config, 'depth_use_normalized_vw', True), device=device)
            for k, v in out.items():
                rendered[k] = v.view(*prefix_rays, *v.shape[1:])
        return raw_ret
