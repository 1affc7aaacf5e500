"""Rendering mixin of the distant-view NeRF++ model -- counterpart of ``NeRFRendererMixinDistant``
(nr3d_lib/models/fields_distant/nerf/renderer_mixin.py:87-540)."""
from typing import Dict, Optional, Tuple

import torch

from nr3d_lib_amd.graphics.nerf.nerf_distant_ray_query import nerf_distant_ray_query, nerf_distant_ray_query_march
from nr3d_lib_amd.graphics.raymarch.nerfpp_raymarch import nerfpp_raymarch

__all__ = ['NeRFRendererMixinDistant']


class NeRFRendererMixinDistant:
    """Put in front of a network class: ``class Model(NeRFRendererMixinDistant, Net)``.  The constructor takes the reference's renderer
    keywords and hands every other keyword to the next class (``super().__init__(**net_kwargs)``); the network provides ``space`` (the
    close-range AABBSpace), ``forward(x=, v=, h_appear=)`` and ``forward_density(x)`` on 4-D inputs.  ``_ray_marching``,
    ``_ray_query_march`` and ``ray_query`` delegate to ``nerfpp_raymarch``, ``nerf_distant_ray_query_march`` and
    ``nerf_distant_ray_query``.

    LEFT OUT: the acceleration structure and the training hooks of the reference's class (``populate``, ``training_initialize``,
    ``training_before_per_step``, ``training_after_per_step``, the sample collection inside ``forward_density``, ``query_density``).
    ``accel_cfg`` is stored and not used; ``ray_test`` raises NotImplementedError as the reference's does."""

    def __init__(self, ray_query_cfg: dict = dict(), accel_cfg: dict = None, radius_scale_min: float = 1.0,
                 radius_scale_max: float = 100.0, include_inf_distance: bool = None, **net_kwargs) -> None:
        mro = type(self).mro()
        assert mro[mro.index(NeRFRendererMixinDistant) + 1] is not object, \
            "NeRFRendererMixinDistant comes before the network class when inheriting and is not instantiated on its own"
        super().__init__(**net_kwargs)
        self.ray_query_cfg = ray_query_cfg
        self.accel_cfg = accel_cfg
        self.accel = None
        self.radius_scale_min = radius_scale_min
        self.radius_scale_max = radius_scale_max
        self.include_inf_distance = include_inf_distance

    def ray_test(self, rays_o: torch.Tensor, rays_d: torch.Tensor, near=None, far=None, **extra_ray_data):
        raise NotImplementedError

    def _ray_marching(self, rays_o: torch.Tensor, rays_d: torch.Tensor, t_min: Optional[torch.Tensor] = None,
                      t_max: Optional[torch.Tensor] = None, perturb: bool = False, max_steps: int = 256, sample_mode: str = "box",
                      interval_type: str = "inverse_proportional"):
        return nerfpp_raymarch(self.space, rays_o, rays_d, t_min, t_max, radius_scale_min=self.radius_scale_min,
                               radius_scale_max=self.radius_scale_max, include_inf_distance=self.include_inf_distance, perturb=perturb,
                               max_steps=max_steps, sample_mode=sample_mode, interval_type=interval_type)

    def _ray_query_march(self, ray_tested: Dict[str, torch.Tensor], *, with_rgb=True, with_normal=False, perturb=False, march_cfg=dict(),
                         compression=True, bypass_sigma_fn=None, bypass_alpha_fn=None) -> Tuple[dict, dict]:
        return nerf_distant_ray_query_march(self, ray_tested, with_rgb=with_rgb, with_normal=with_normal, perturb=perturb,
                                            march_cfg=march_cfg, compression=compression, bypass_sigma_fn=bypass_sigma_fn,
                                            bypass_alpha_fn=bypass_alpha_fn)

    def ray_query(self, ray_input: Dict[str, torch.Tensor] = None, ray_tested: Dict[str, torch.Tensor] = None, config=dict(),
                  return_buffer=False, return_details=False, render_per_obj_individual=False):
        return nerf_distant_ray_query(self, ray_input=ray_input, ray_tested=ray_tested, config=config, return_buffer=return_buffer,
                                      return_details=return_details, render_per_obj_individual=render_per_obj_individual)
