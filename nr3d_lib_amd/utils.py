"""Helpers of the reference's nr3d_lib/utils.py that this package needs."""
from typing import Literal

import torch

__all__ = ['torch_consecutive_nearest1d', 'nearest_keyframe_index']


def nearest_keyframe_index(ts_keyframes: torch.Tensor, ts: torch.Tensor) -> torch.Tensor:
    """``torch_consecutive_nearest1d(ts_keyframes, ts)[0]`` alone: one launch for float32 GPU input"""
    if ts_keyframes.is_cuda and ts.is_cuda and ts_keyframes.dtype == torch.float32 and ts.dtype == torch.float32:
        from nr3d_lib_amd.bindings import _occ_grid
        return _occ_grid.nearest_keyframe(ts_keyframes.contiguous(), ts.contiguous())
    return torch_consecutive_nearest1d(ts_keyframes, ts)[0]


def torch_consecutive_nearest1d(seq_1d_sorted: torch.Tensor, t: torch.Tensor, *,
                                mode: Literal['nearest', 'ceil', 'floor'] = 'nearest'):
    """For every value of ``t`` its nearest neighbour in the sorted 1-D sequence ``seq_1d_sorted``
    (nr3d_lib/utils.py:675-699) -> (closest_inds int64, closest_mask bool: the previous entry is strictly closer, closest_dis).
    float32 GPU input takes the index from one launch (bindings._occ_grid.nearest_keyframe: the same float32 operations in
    the same order); the mask and the distance follow from it.  Anything else runs the reference's torch ops."""
    assert seq_1d_sorted.dim() == 1, "`seq_1d_sorted` must be 1D sequences"
    assert seq_1d_sorted.is_contiguous(), "Please make sure input is_contiguous()"
    if mode in ('ceil', 'floor'):
        raise NotImplementedError
    if mode != 'nearest':
        raise RuntimeError(f"Invalid mode={mode}")
    if seq_1d_sorted.is_cuda and t.is_cuda and seq_1d_sorted.dtype == torch.float32 and t.dtype == torch.float32 \
            and len(seq_1d_sorted) >= 1:
        from nr3d_lib_amd.bindings import _occ_grid
        closest_inds = _occ_grid.nearest_keyframe(seq_1d_sorted, t.contiguous())
        if len(seq_1d_sorted) == 1:
            closest_mask = torch.zeros_like(closest_inds, dtype=torch.bool)
        else:
            # the previous entry was chosen exactly when the result is not the clamped searchsorted index itself
            inds = torch.searchsorted(seq_1d_sorted, t).clamp(1, len(seq_1d_sorted) - 1)
            closest_mask = closest_inds != inds
        closest_dis = (seq_1d_sorted[closest_inds] - t).abs()
        return closest_inds, closest_mask, closest_dis
    return _nearest1d_torch(seq_1d_sorted, t)


def _nearest1d_torch(seq_1d_sorted: torch.Tensor, t: torch.Tensor):
    """the reference's own ops (the 'nearest' branch of nr3d_lib/utils.py:683-699)"""
    inds = torch.searchsorted(seq_1d_sorted, t)
    inds = inds.clamp(1, len(seq_1d_sorted) - 1)
    prev_dis = (seq_1d_sorted[inds - 1] - t).abs()
    next_dis = (seq_1d_sorted[inds] - t).abs()
    closest_mask = prev_dis < next_dis
    closest_dis = torch.where(closest_mask, prev_dis, next_dis)
    closest_inds = torch.where(closest_mask, inds - 1, inds)
    return closest_inds, closest_mask, closest_dis
