"""Depth samplers on rays -- counterpart of the parts of nr3d_lib/graphics/raysample.py the hot-path drivers use:
``packed_sample_cdf`` / ``packed_sample_pdf`` (:38-84, on the HIP ``packed_invert_cdf``), the batched inverse-CDF samplers
``batch_sample_cdf`` / ``batch_sample_pdf`` (:221-282, plain torch), the three ``batch_sample_step_*`` ladders (:285-383) and the
linear stepper inside packed segments (:161-205, ``_v1``) that ``ForestBlockSpace.ray_step_coarse(step_mode='linear')`` calls.
Same names, arguments and return conventions."""
from typing import Tuple, Union

import torch

from nr3d_lib_amd.graphics.pack_ops import (get_pack_infos_from_n, interleave_arange_simple, interleave_linstep, packed_cumsum,
                                            packed_diff, packed_div, packed_invert_cdf)

__all__ = ['packed_sample_cdf', 'packed_sample_pdf', 'batch_sample_cdf', 'batch_sample_pdf', 'batch_sample_step_linear',
           'batch_sample_step_wrt_depth', 'batch_sample_step_wrt_sqrt_depth',
           'interleave_sample_step_linear_in_packed_segments']


def _per_ray(near, far, prefix_shape):
    if prefix_shape is None:
        prefix_shape = [1] if list(near.shape) == [1] else near.squeeze().shape
    shp = tuple(prefix_shape)
    return near.squeeze().expand(shp).unsqueeze(-1), far.squeeze().expand(shp).unsqueeze(-1), shp


def _steps(num_samples, shp, perturb, like, first=0):
    """{first, first+1, ...} (+ U(0,1) per sample when perturbing)"""
    idx = torch.arange(first, first + num_samples, device=like.device)
    if perturb:
        idx = idx + torch.rand((*shp, num_samples), dtype=like.dtype, device=like.device)
    return idx


def _with_deltas(t, last):
    """interval lengths: differences, the last one given by `last` (a tensor) or repeated (None)"""
    d = torch.zeros_like(t)
    d[..., :-1] = torch.diff(t, dim=-1)
    d[..., -1] = d[..., -2] if last is None else last
    return d


def batch_sample_step_linear(near, far, num_samples: int, prefix_shape=None, perturb=False, return_dt=False):
    """uniform in depth; perturb: one uniform sample per stratum (raysample.py:285-311)"""
    near, far, shp = _per_ray(near, far, prefix_shape)
    dt = (far - near) / (num_samples if perturb else num_samples - 1)
    t = torch.addcmul(near, _steps(num_samples, shp, perturb, near).to(near.dtype), dt)
    if not return_dt:
        return t
    return t, (_with_deltas(t, (far[..., 0] - near[..., 0]) / num_samples) if perturb else dt.expand((*shp, num_samples)))


@torch.no_grad()
def _geometric(near, far, num_samples, shp, perturb):
    n = num_samples if perturb else num_samples - 1
    logk = torch.log(far / near) / n                          # far / near must be finite: callers clamp it
    first = -num_samples if perturb else 1 - num_samples
    return far * torch.exp(logk * _steps(num_samples, logk.shape[:-1], perturb, near, first=first))


@torch.no_grad()
def batch_sample_step_wrt_depth(near, far, num_samples: int, prefix_shape=None, perturb=False, return_dt=False):
    """step proportional to depth (geometric ladder with ratio clamped to num_samples, raysample.py:342-362)"""
    near, far, shp = _per_ray(near, far, prefix_shape)
    ratio = (far / near).clamp_max(num_samples)
    near_ = far / ratio
    t = _geometric(near_, far, num_samples, shp, perturb)
    t = (t - near_) * ((far - near) / (far - near_)) + near
    return (t, _with_deltas(t, None)) if return_dt else t


@torch.no_grad()
def batch_sample_step_wrt_sqrt_depth(near, far, num_samples: int, prefix_shape=None, perturb=False, return_dt=False):
    """step proportional to sqrt(depth): t = (k i + c)^2 / 4 (raysample.py:364-383)"""
    near, far, shp = _per_ray(near, far, prefix_shape)
    c = (4 * near).sqrt()
    k = ((4 * far).sqrt() - c) / (num_samples if perturb else num_samples - 1)
    t = 0.25 * (k * _steps(num_samples, shp, perturb, near) + c).square()
    return (t, _with_deltas(t, None)) if return_dt else t


def packed_sample_cdf(bins: torch.Tensor, cdfs: torch.Tensor, pack_infos: torch.Tensor, num_to_sample: int,
                      perturb=False) -> Tuple[torch.Tensor, torch.Tensor]:
    """inverse-CDF sampling per pack: bins / cdfs packed [num_pts] (cdf with a leading zero per pack) ->
    (t_samples, global bin index) both [num_packs, num_to_sample] (raysample.py:38-62)"""
    n_packs = pack_infos.shape[0]
    if perturb:
        u = batch_sample_step_linear(bins.new_zeros(n_packs), bins.new_ones(n_packs), num_to_sample, perturb=True)
    else:
        u = torch.linspace(0., 1., num_to_sample + 2, device=bins.device, dtype=bins.dtype)[1:-1].expand(n_packs, num_to_sample)
    return packed_invert_cdf(bins, cdfs.to(bins.dtype), u.contiguous(), pack_infos)


@torch.no_grad()
def packed_sample_pdf(bins: torch.Tensor, weights: torch.Tensor, pack_infos: torch.Tensor, num_to_sample: int,
                      perturb=False) -> Tuple[torch.Tensor, torch.Tensor]:
    """``packed_sample_cdf`` on the normalised exclusive cumsum of the interval weights (packed [num_pts], trailing zero in every
    pack) (raysample.py:64-84)"""
    cdfs = packed_cumsum(weights, pack_infos, exclusive=True)
    last = cdfs[pack_infos[..., 0] + pack_infos[..., 1] - 1]
    return packed_sample_cdf(bins, packed_div(cdfs, last.clamp_min(1e-5), pack_infos), pack_infos, num_to_sample, perturb=perturb)


def cdf_positions(like: torch.Tensor, prefix, num_to_sample: int, perturb: bool) -> torch.Tensor:
    """the positions in (0, 1) the batched samplers invert the CDF at: one shared row [num_to_sample] of interior linspace
    points, or with ``perturb`` one stratified (hence sorted) row per ray [*prefix, num_to_sample]"""
    if perturb:
        return batch_sample_step_linear(like.new_zeros(prefix), like.new_ones(prefix), num_to_sample, perturb=True).contiguous()
    return torch.linspace(0., 1., num_to_sample + 2, device=like.device, dtype=like.dtype)[1:-1].contiguous()


@torch.no_grad()
def batch_sample_cdf(bins: torch.Tensor, cdf: torch.Tensor, num_to_sample: int, perturb=False, eps: float = 1e-5) -> torch.Tensor:
    """inverse-CDF sampling per ray: bins, cdf [..., n] (cdf with a leading zero) -> t [..., num_to_sample] (raysample.py:221-259)"""
    u = cdf_positions(bins, bins.shape[:-1], num_to_sample, perturb).expand((*bins.shape[:-1], num_to_sample)).contiguous()
    inds = torch.searchsorted(cdf.detach(), u, right=False)
    below, above = (inds - 1).clamp_min(0), inds.clamp_max(cdf.shape[-1] - 1)
    cdf_lo, cdf_hi = cdf.gather(-1, below), cdf.gather(-1, above)
    bins_lo, bins_hi = bins.gather(-1, below), bins.gather(-1, above)
    denom = cdf_hi - cdf_lo
    denom[denom < eps] = 1
    return bins_lo + (u - cdf_lo) / denom * (bins_hi - bins_lo)


@torch.no_grad()
def batch_sample_pdf(bins: torch.Tensor, weights: torch.Tensor, num_to_sample: int, perturb=False, eps=1e-5) -> torch.Tensor:
    """bins [..., n], interval weights [..., n-1] -> t [..., num_to_sample] (raysample.py:262-282)"""
    pdf = weights / torch.sum(weights, -1, keepdim=True).clamp_min(eps)
    cdf = torch.cat([pdf.new_zeros((*pdf.shape[:-1], 1)), torch.cumsum(pdf, -1)], -1)
    return batch_sample_cdf(bins, cdf, num_to_sample, perturb, eps)


@torch.no_grad()
def interleave_sample_step_linear_in_packed_segments(
        near: Union[torch.Tensor, float], far: Union[torch.Tensor, float], entry: torch.Tensor, exit: torch.Tensor,
        seg_pack_infos: torch.Tensor, step_size: float = 0.01, step_size_factor: float = 1.0, min_steps: int = 2,
        max_steps: int = 512, perturb=False):
    """equal steps inside every (entry, exit) segment of every ray, on the ray's own ladder near + k step_size
    (raysample.py:161-205, ``interleave_sample_step_linear_in_packed_segments_v1``): a segment takes the rungs from
    trunc((entry - near) / step) up to and including trunc((exit - near) / step) -- without the last one when perturbing, every
    sample then moves by U(0, 1) steps -- clamped to [min_steps, max_steps] rungs counted from the first.  ``far`` is not used, as
    in the reference.
    -> (t_samples, deltas, ridx, ray_pack_infos, sidx, out_seg_pack_infos): flat per sample the depth, the step to the next sample
    (``step_size`` without perturb, and for the last sample of a segment), the ray and the segment; the packs per ray and per
    segment"""
    num_rays = seg_pack_infos.shape[0]
    near = entry.new_full([num_rays], near) if not isinstance(near, torch.Tensor) else near
    step_size = step_size * step_size_factor
    _, seg_ridx = interleave_arange_simple(seg_pack_infos[..., 1].contiguous())
    _near = near[seg_ridx]
    entry_ind = (entry - _near).div_(step_size, rounding_mode='trunc').long()
    exit_ind = (exit - _near).div_(step_size, rounding_mode='trunc').long()
    if not perturb:
        exit_ind.add_(1)
    n_per_seg = (exit_ind - entry_ind).clamp_(min_steps, max_steps)
    out_seg_pack_infos = get_pack_infos_from_n(n_per_seg)
    indexing, sidx = interleave_linstep(entry_ind, n_per_seg, 1, return_idx=True)
    if not perturb:
        t_samples = _near[sidx] + indexing.to(near.dtype) * step_size
        deltas = near.new_full(sidx.shape, step_size)
    else:
        indexing = indexing.to(near.dtype) + torch.rand_like(indexing, dtype=near.dtype, device=near.device)
        t_samples = _near[sidx] + indexing * step_size
        last_inds = out_seg_pack_infos[..., 0] + out_seg_pack_infos[..., 1] - 1
        deltas = packed_diff(t_samples, out_seg_pack_infos).index_fill_(0, last_inds, step_size)
    ridx = seg_ridx[sidx]
    n_per_ray = seg_pack_infos.new_zeros([num_rays])
    n_per_ray.index_add_(0, seg_ridx, n_per_seg)
    return t_samples, deltas, ridx, get_pack_infos_from_n(n_per_ray), sidx, out_seg_pack_infos
