"""Occupancy-grid acceleration of ONE time-varying box (``AABBDynamicSpace``): one grid per keyframe, every ray / point uses
the grid of the keyframe nearest to its timestamp.

Counterpart of the reference's nr3d_lib/models/accelerations/occgrid_accel/dynamic.py: ``OccGridAccelDynamic`` (:25-170, the
keyframes as the entries of an ``OccGridEmaBatched``) and ``OccGridAccelStaticAndDynamic`` (:201-401, a static ``OccGridEma``
OR-ed onto every keyframe's grid).  Both march through ``occgrid_raymarch_dynamic``, which with ``FUSED_DYNAMIC_MARCH`` looks the
frame up and ORs the static grid inside the marcher -- ``ray_march`` then never builds the [T, Rx, Ry, Rz] union that
``get_occ_grid()`` of the combined accel still returns.  ``debug_vis`` is not provided.
"""
import math
from numbers import Number
from typing import Dict, List, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from nr3d_lib_amd.graphics.raymarch import RaymarchRetDynamic
from nr3d_lib_amd.graphics.raymarch.occgrid_raymarch import occgrid_raymarch_dynamic
from nr3d_lib_amd.models.accelerations.occgrid import OccGridEma, OccGridEmaBatched
from nr3d_lib_amd.models.accelerations.occgrid_accel.single import OccGridAccel
from nr3d_lib_amd.models.spatial import AABBDynamicSpace, AABBSpace
from nr3d_lib_amd.utils import nearest_keyframe_index

__all__ = ['OccGridAccelDynamic', 'OccGridAccelStaticAndDynamic']


def _keyframes(ts_keyframes, device) -> torch.Tensor:
    if isinstance(ts_keyframes, torch.Tensor):
        return ts_keyframes.to(device=device).contiguous()
    return torch.tensor(np.asarray(ts_keyframes, dtype=np.float32), device=device)


def _stats(t: torch.Tensor, prefix: str) -> Dict[str, Number]:
    """mean / min / max / std of a (possibly empty) tensor, as the reference's tensor_statistics with these metrics"""
    t = t.float()
    if t.numel() == 0:
        return {f'{prefix}.{m}': 0. for m in ('mean', 'min', 'max', 'std')}
    return {f'{prefix}.mean': t.mean().item(), f'{prefix}.min': t.min().item(), f'{prefix}.max': t.max().item(),
            f'{prefix}.std': t.std().item() if t.numel() > 1 else 0.}


def _per_frame_stats(occ_grid: torch.Tensor, prefix: str = '') -> Dict[str, Number]:
    num = occ_grid.sum().item()
    per_frame = occ_grid.sum(dim=tuple(range(1, occ_grid.dim())))
    nonempty = per_frame[per_frame != 0]
    return {f'{prefix}num_occ': num, f'{prefix}frac_occ': num / occ_grid.numel(),
            f'{prefix}num_empty_frame': (per_frame == 0).sum().item(),
            **_stats(nonempty, f'{prefix}per_frame.nonempty.num_occupied'),
            **_stats(nonempty / math.prod(occ_grid.shape[1:]), f'{prefix}per_frame.nonempty.frac_occupied')}


class _DynamicBase(nn.Module):
    is_dynamic = True       # graphics._ray_query._march passes ray_tested['rays_ts']

    def _setup(self, space, ts_keyframes, resolution, vox_size, dtype, device):
        assert isinstance(space, AABBDynamicSpace), f"{self.__class__.__name__} expects space of AABBDynamicSpace"
        self.space, self.dtype = space, dtype
        self.num_frames = len(ts_keyframes)
        self.register_buffer('ts_keyframes', _keyframes(ts_keyframes, device), persistent=True)
        assert (resolution is not None) != (vox_size is not None), "Please specify `vox_size` or `resolution` for OccGridAccel."
        self.training_granularity = 0.0
        return (self.space.radius3d * 2 / vox_size).long() if resolution is None else resolution

    device = property(lambda self: self.space.device)

    def _with_ts(self, val_query_fn_normalized_x_ts):
        def converted(x, *, bidx=...):          # the grid stack's `bidx` is the frame index
            return val_query_fn_normalized_x_ts(x, ts=self.ts_keyframes[bidx])
        return converted

    def _march(self, occ_dynamic, occ_static, rays_o, rays_d, rays_ts, near, far, perturb, normalized, march_cfg):
        if not normalized:
            rays_o, rays_d = self.space.normalize_rays(rays_o, rays_d)
        return occgrid_raymarch_dynamic(occ_dynamic, self.ts_keyframes, rays_o, rays_d, rays_ts, near, far,
                                        occ_grid_static=occ_static, perturb=perturb, **march_cfg)


class OccGridAccelDynamic(_DynamicBase):
    def __init__(self, space: AABBDynamicSpace, ts_keyframes: torch.Tensor,
                 resolution: Union[int, List[int], torch.Tensor] = None, vox_size: float = None, dtype=torch.float, device=None,
                 **occ_kwargs) -> None:
        super().__init__()
        resolution = self._setup(space, ts_keyframes, resolution, vox_size, dtype, device)
        self.occ = OccGridEmaBatched(num_batches=self.num_frames, resolution=resolution, **occ_kwargs, dtype=dtype, device=device)

    NUM_DIM = property(lambda self: self.occ.NUM_DIM)
    resolution = property(lambda self: self.occ.resolution)

    def get_occ_grid(self):
        return self.occ.occ_grid

    @torch.no_grad()
    def init(self, val_query_fn_normalized_x_ts, logger=None):
        return self.occ.init(self._with_ts(val_query_fn_normalized_x_ts), logger=logger)

    @torch.no_grad()
    def step(self, cur_it: int, val_query_fn_normalized_x_ts, logger=None):
        return self.occ.step(cur_it, self._with_ts(val_query_fn_normalized_x_ts), logger=logger)

    @torch.no_grad()
    def collect_samples(self, pts: torch.Tensor, ts: torch.Tensor, val: torch.Tensor, normalized=True):
        """forward-hook style: the samples feed the grid of the keyframe nearest to each sample's timestamp"""
        if self.training:
            if not normalized:
                pts = self.space.normalize_coords(pts)
            self.occ.collect_samples(pts, nearest_keyframe_index(self.ts_keyframes, ts), val)

    @torch.no_grad()
    def sample_pts_in_occupied(self, num_pts: int) -> Tuple[torch.Tensor, torch.Tensor]:
        pts, fidx = self.occ.sample_pts_in_occupied(num_pts)
        return pts, self.ts_keyframes[fidx]

    @torch.no_grad()
    def query_occupancy(self, pts: torch.Tensor, ts: torch.Tensor) -> torch.BoolTensor:
        """pts in [-1, 1]"""
        return self.occ.query(pts, nearest_keyframe_index(self.ts_keyframes, ts))

    def ray_march(self, rays_o: torch.Tensor, rays_d: torch.Tensor, rays_ts: torch.Tensor, near=None, far=None, *, perturb=False,
                  normalized=True, step_size: float = 1e-3, max_step_size: float = 1e10, dt_gamma: float = 0.0,
                  max_steps: int = 512) -> RaymarchRetDynamic:
        return self._march(self.get_occ_grid(), None, rays_o, rays_d, rays_ts, near, far, perturb, normalized,
                           dict(step_size=step_size, max_step_size=max_step_size, dt_gamma=dt_gamma, max_steps=max_steps))

    @torch.no_grad()
    def debug_stats(self) -> Dict[str, Number]:
        return _per_frame_stats(self.get_occ_grid())


class OccGridAccelStaticAndDynamic(_DynamicBase):
    """combined occupancy: a static grid and one dynamic grid per keyframe; a cell is occupied when either is"""

    def __init__(self, space: AABBDynamicSpace, ts_keyframes: torch.Tensor,
                 resolution: Union[int, List[int], torch.Tensor] = None, vox_size: float = None, occ_static_cfg: dict = ...,
                 occ_dynamic_cfg: dict = ..., dtype=torch.float, device=None, **occ_common_kwargs) -> None:
        super().__init__()
        resolution = self._setup(space, ts_keyframes, resolution, vox_size, dtype, device)
        self.occ = None
        self.occ_static = OccGridEma(resolution=resolution, **occ_static_cfg, **occ_common_kwargs, dtype=dtype, device=device)
        self.occ_dynamic = OccGridEmaBatched(num_batches=self.num_frames, resolution=resolution, **occ_dynamic_cfg,
                                             **occ_common_kwargs, dtype=dtype, device=device)

    NUM_DIM = property(lambda self: self.occ_static.NUM_DIM)
    resolution = property(lambda self: self.occ_static.resolution)

    def get_occ_grid(self):
        """the materialised union [T, Rx, Ry, Rz] (``ray_march`` does not need it on the fused route)"""
        dyn = self.occ_dynamic.occ_grid
        return dyn | self.occ_static.occ_grid.unsqueeze(0).expand_as(dyn)

    @torch.no_grad()
    def init(self, val_query_fn_static_normalized_x, val_query_fn_dynamic_normalized_x_ts, logger=None):
        updated = self.occ_dynamic.init(self._with_ts(val_query_fn_dynamic_normalized_x_ts), logger=logger)
        updated |= self.occ_static.init(val_query_fn_static_normalized_x, logger=logger)
        return updated

    @torch.no_grad()
    def step(self, cur_it: int, val_query_fn_static_normalized_x, val_query_fn_dynamic_normalized_x_ts, logger=None):
        updated = self.occ_dynamic.step(cur_it, self._with_ts(val_query_fn_dynamic_normalized_x_ts), logger=logger)
        updated |= self.occ_static.step(cur_it, val_query_fn_static_normalized_x, logger=logger)
        return updated

    @torch.no_grad()
    def collect_samples(self, pts: torch.Tensor, ts: torch.Tensor, val_static: torch.Tensor, val_dynamic: torch.Tensor,
                        normalized=True):
        if self.training:
            if not normalized:
                pts = self.space.normalize_coords(pts)
            self.occ_dynamic.collect_samples(pts, nearest_keyframe_index(self.ts_keyframes, ts), val_dynamic)
            self.occ_static.collect_samples(pts, val_static)

    @torch.no_grad()
    def sample_pts_in_occupied(self, num_pts: int) -> Tuple[torch.Tensor, torch.Tensor]:
        raise NotImplementedError

    @torch.no_grad()
    def query_occupancy(self, pts: torch.Tensor, ts: torch.Tensor) -> torch.BoolTensor:
        """pts in [-1, 1]"""
        fidx = nearest_keyframe_index(self.ts_keyframes, ts)
        return self.occ_static.query(pts) | self.occ_dynamic.query(pts, fidx)

    def ray_march(self, rays_o: torch.Tensor, rays_d: torch.Tensor, rays_ts: torch.Tensor, near=None, far=None, *, perturb=False,
                  normalized=True, step_size: float = 1e-3, max_step_size: float = 1e10, dt_gamma: float = 0.0,
                  max_steps: int = 512) -> RaymarchRetDynamic:
        return self._march(self.occ_dynamic.occ_grid, self.occ_static.occ_grid, rays_o, rays_d, rays_ts, near, far, perturb,
                           normalized, dict(step_size=step_size, max_step_size=max_step_size, dt_gamma=dt_gamma, max_steps=max_steps))

    def get_accel_static(self):
        """a fresh single-grid accel over the same box"""
        space = AABBSpace(aabb=self.space.aabb, dtype=self.dtype, device=self.device)
        return OccGridAccel(space=space, resolution=self.resolution, dtype=self.dtype, device=self.device)

    def get_accel_dynamic(self):
        """a fresh per-keyframe accel over the same box and keyframes"""
        return OccGridAccelDynamic(space=self.space, ts_keyframes=self.ts_keyframes, resolution=self.resolution, dtype=self.dtype,
                                   device=self.device)

    @torch.no_grad()
    def debug_stats(self) -> Dict[str, Number]:
        static = self.occ_static.occ_grid
        num = static.sum().item()
        return {'static.num_occupied': num, 'static.frac_occupied': num / static.numel(),
                **_per_frame_stats(self.occ_dynamic.occ_grid, 'dynamic.')}
