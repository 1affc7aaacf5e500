"""Occupancy-grid acceleration for a batch of TIME-VARYING objects in one shared box (``BatchedDynamicSpace``): one grid per
(instance, keyframe), flattened as slice = instance * num_frames + frame.

Counterpart of the reference's nr3d_lib/models/accelerations/occgrid_accel/batched_dynamic.py: the operations on the current
batch (``OccGridAccelBatchedDynamic_Base`` :24-110) and the persistent EMA grids (``OccGridAccelBatchedDynamic_Ema`` :112-255).
The march is ``occgrid_raymarch_dynamic`` with per-ray batch indices: the frame lookup, the slice index and the split of the
flat slice into (batch, timestamp) per sample happen inside the marcher on the fused route.  ``_Getter`` and ``debug_vis`` are
not provided.
"""
import math
from numbers import Number
from typing import Dict, List, Tuple, Union

import torch
import torch.nn as nn

from nr3d_lib_amd.graphics.raymarch import RaymarchRetBatchedDynamic
from nr3d_lib_amd.graphics.raymarch.occgrid_raymarch import occgrid_raymarch_dynamic
from nr3d_lib_amd.models.accelerations.occgrid import OccGridEmaBatched, err_msg_empty_occ, sample_pts_in_voxels
from nr3d_lib_amd.models.spatial import BatchedDynamicSpace
from nr3d_lib_amd.utils import nearest_keyframe_index

from .dynamic import _keyframes, _stats

__all__ = ['OccGridAccelBatchedDynamic_Base', 'OccGridAccelBatchedDynamic_Ema']


class OccGridAccelBatchedDynamic_Base(nn.Module):
    """operations on the grids of the CURRENT batch (``tmp_flat_occ_grid`` [B * num_frames, Rx, Ry, Rz], set by set_condition)"""
    is_dynamic = True       # graphics._ray_query._march passes rays_bidx AND rays_ts
    tmp_flat_occ_grid: torch.Tensor = None

    def _grids(self, what: str) -> torch.Tensor:
        assert self.tmp_flat_occ_grid is not None, f"Please call set_condition() first before {what}()"
        return self.tmp_flat_occ_grid

    def _split(self, flat_bidx: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """flat slice index -> (batch index, frame index)"""
        bidx = torch.div(flat_bidx, self.num_frames, rounding_mode='floor').long()
        return bidx, flat_bidx - bidx * self.num_frames

    @torch.no_grad()
    def cur_batch__sample_pts_in_occupied(self, num_pts: int) -> Tuple[torch.Tensor, torch.LongTensor, torch.Tensor]:
        """uniform points in the occupied voxels of the current batch -> (pts in [-1, 1], local batch index, ts)"""
        occupied = self._grids("sample_pts_in_occupied").nonzero().long()
        assert occupied.numel() > 0, err_msg_empty_occ
        pts, vidx = sample_pts_in_voxels(occupied[..., 1:], num_pts, resolution=self.resolution, dtype=self.dtype)
        bidx, fidx = self._split(occupied[..., 0][vidx])
        return pts, bidx, self.ts_keyframes[fidx]

    @torch.no_grad()
    def cur_batch__query_occupancy(self, pts: torch.Tensor, bidx: torch.LongTensor, ts: torch.Tensor) -> torch.BoolTensor:
        """pts in [-1, 1] with their local batch index and timestamp -> occupied?"""
        grids = self._grids("query_occupancy")
        res = self.resolution
        gidx = ((pts / 2. + 0.5) * res).long().clamp(res.new_tensor([0]), res - 1)
        flat_bidx = bidx * self.num_frames + nearest_keyframe_index(self.ts_keyframes, ts)
        return grids[(flat_bidx,) + tuple(gidx.movedim(-1, 0))]

    def cur_batch__ray_march(self, rays_o: torch.Tensor, rays_d: torch.Tensor, rays_bidx: torch.Tensor, rays_ts: torch.Tensor, *,
                             near=None, far=None, perturb=False, step_size: float = 1e-3, max_step_size: float = 1e10,
                             dt_gamma: float = 0.0, max_steps: int = 512) -> RaymarchRetBatchedDynamic:
        grids = self._grids("ray_march")
        return occgrid_raymarch_dynamic(grids, self.ts_keyframes, rays_o, rays_d, rays_ts, near, far, rays_bidx=rays_bidx,
                                        num_batches=grids.shape[0] // self.num_frames, perturb=perturb, step_size=step_size,
                                        max_step_size=max_step_size, dt_gamma=dt_gamma, max_steps=max_steps)


class OccGridAccelBatchedDynamic_Ema(OccGridAccelBatchedDynamic_Base):
    """one persistent EMA grid per (instance, keyframe); a batch selects its instances' grids"""

    def __init__(self, space: BatchedDynamicSpace, num_batches: int, ts_keyframes: torch.Tensor,
                 resolution: Union[int, List[int], torch.Tensor] = None, dtype=torch.float, device=None, **occ_kwargs) -> None:
        super().__init__()
        assert isinstance(space, BatchedDynamicSpace), f"{self.__class__.__name__} expects space of BatchedDynamicSpace"
        self.space, self.dtype = space, dtype
        self.training_granularity = 0.0
        self.num_frames, self.num_batches_real = len(ts_keyframes), num_batches
        self.register_buffer('ts_keyframes', _keyframes(ts_keyframes, device), persistent=True)
        self.occ = OccGridEmaBatched(resolution=resolution, **occ_kwargs, num_batches=num_batches * self.num_frames, dtype=dtype,
                                     device=device)
        self.clean_condition()

    device = property(lambda self: self.space.device)
    NUM_DIM = property(lambda self: self.occ.NUM_DIM)
    resolution = property(lambda self: self.occ.resolution)

    def get_occ_grid(self):
        return self.occ.occ_grid

    def set_condition(self, batch_size: int, *, ins_inds_per_batch: torch.LongTensor = None, val_query_fn_normalized_x_bi_ts=None):
        assert ins_inds_per_batch is not None, f"`ins_inds_per_batch` is required for {type(self)}"
        self.batch_size, self.ins_inds_per_batch = batch_size, ins_inds_per_batch
        frames = torch.arange(self.num_frames, device=self.device, dtype=torch.long)
        self.tmp_flat_bidx = (ins_inds_per_batch.unsqueeze(1) * self.num_frames + frames.unsqueeze(0)).flatten()
        unflat = self.get_occ_grid().unflatten(0, (self.num_batches_real, self.num_frames))
        self.tmp_flat_occ_grid = unflat[ins_inds_per_batch, :].flatten(0, 1).contiguous()

    def clean_condition(self):
        self.batch_size = self.ins_inds_per_batch = self.tmp_flat_bidx = self.tmp_flat_occ_grid = None

    def _with_bi_ts(self, val_query_fn_normalized_x_bi_ts):
        def converted(x, *, bidx=...):          # the grid stack's `bidx` is the flat slice index
            real_bidx, fidx = self._split(bidx)
            return val_query_fn_normalized_x_bi_ts(x, bidx=real_bidx, ts=self.ts_keyframes[fidx])
        return converted

    @torch.no_grad()
    def init(self, val_query_fn_normalized_x_bi_ts, logger=None):
        assert self.batch_size is not None and self.batch_size == self.num_batches_real, \
            "Before init(), should set_condition() on all batches (i.e. all latents)."
        return self.occ.init(self._with_bi_ts(val_query_fn_normalized_x_bi_ts), logger=logger)

    @torch.no_grad()
    def cur_batch__step(self, cur_it: int, val_query_fn_normalized_x_bi_ts, logger=None):
        assert self.ins_inds_per_batch is not None, "Please call set_condition() first before step()"
        return self.occ.step(cur_it, self._with_bi_ts(val_query_fn_normalized_x_bi_ts), within_bi=self.tmp_flat_bidx, logger=logger)

    @torch.no_grad()
    def cur_batch__collect_samples(self, pts: torch.Tensor, bidx: torch.LongTensor, ts: torch.Tensor, val: torch.Tensor,
                                   normalized=True):
        """forward-hook style: the field's samples of this batch (local ``bidx``) feed the grid of their instance and keyframe"""
        if self.training:
            assert self.ins_inds_per_batch is not None, "Please call set_condition() first before collect_samples()"
            if not normalized:
                pts = self.space.cur_batch__normalize_coords(pts, bidx)
            fidx = nearest_keyframe_index(self.ts_keyframes, ts)
            self.occ.collect_samples(pts, self.ins_inds_per_batch[bidx] * self.num_frames + fidx, val)

    @torch.no_grad()
    def debug_stats(self) -> Dict[str, Number]:
        occ_grid = self.get_occ_grid()
        unflat = occ_grid.unflatten(0, (self.num_batches_real, self.num_frames))
        per_ins = unflat.sum(dim=tuple(range(2, self.NUM_DIM + 2))).sum(dim=1)
        num = per_ins.sum().item()
        nonempty = per_ins[per_ins != 0]
        return {'num_occ': num, 'frac_occ': num / occ_grid.numel(), 'num_empty_ins': (per_ins == 0).sum().item(),
                **_stats(nonempty, 'per_ins.nonempty.num_occupied'),
                **_stats(nonempty / math.prod(unflat.shape[1:]), 'per_ins.nonempty.frac_occupied')}
