"""Ray marching through binary occupancy grids -- counterpart of the reference's
nr3d_lib/graphics/raymarch/occgrid_raymarch.py (occgrid_raymarch :25-112, occgrid_raymarch_batched :114-221).

Same signatures, same returned records (including the reference's quirk that the single-grid variant
reports the UN-perturbed ``t_starts`` as ``depth_samples`` while the batched one reports ``t_samples``).
"""
from enum import Enum
from typing import Literal, Union

import torch

from nr3d_lib_amd.graphics.pack_ops import get_pack_infos_from_boundary, mark_pack_boundaries, packed_diff
from nr3d_lib_amd.graphics.raymarch import (RaymarchRetBatched, RaymarchRetBatchedDynamic, RaymarchRetDynamic,
                                            RaymarchRetForest, RaymarchRetSingle)
import nr3d_lib_amd.bindings._occ_grid as _backend
from nr3d_lib_amd.utils import _nearest1d_torch

__all__ = ['ContractionType', 'occgrid_raymarch', 'occgrid_raymarch_batched', 'occgrid_raymarch_forest',
           'occgrid_raymarch_dynamic']


class ContractionType(Enum):
    AABB = int(_backend.ContractionType.AABB)
    UN_BOUNDED_TANH = int(_backend.ContractionType.UN_BOUNDED_TANH)
    UN_BOUNDED_SPHERE = int(_backend.ContractionType.UN_BOUNDED_SPHERE)


_CONTRACTIONS = {'aabb': ContractionType.AABB, 'sphere': ContractionType.UN_BOUNDED_SPHERE,
                 'tanh': ContractionType.UN_BOUNDED_TANH}


def _contraction(name):
    try:
        return _backend.ContractionType(_CONTRACTIONS[name.lower()].value)
    except KeyError:
        raise RuntimeError(f"Invalid constraction={name}")


def _as_depth(v, like):
    return v if isinstance(v, torch.Tensor) else like.new_full(like.shape[:-1], v)


# True: the un-jittered post-processing runs as two kernels of the library (bindings._occ_grid.ray_marching_finished);
# False: the reference's op chain below (kept for jitter-after-march and as the cross-check of the fused path)
FUSED_FINISH = True


def _finish(rays_o, rays_d, pack_infos, t_starts, t_ends, ridx, perturb_after):
    """shared post-processing of the raw marcher outputs"""
    ridx = ridx.long()
    ridx_hit = pack_infos[..., 1].nonzero().long()[..., 0].contiguous()
    if ridx_hit.numel() == 0:
        return None
    pack_infos = pack_infos[ridx_hit].contiguous().long()
    t_starts, t_ends = t_starts.squeeze_(-1), t_ends.squeeze_(-1)
    deltas = t_ends - t_starts
    if perturb_after:
        # jitter inside each interval; the deltas are then re-derived as differences (last of a pack = 0)
        t_samples = torch.addcmul(t_starts, torch.rand_like(deltas), deltas)
        deltas = packed_diff(t_samples, pack_infos)
    else:
        t_samples = t_starts
    samples = torch.addcmul(rays_o.index_select(0, ridx), rays_d.index_select(0, ridx), t_starts.unsqueeze(-1))
    return ridx_hit, samples, t_starts, t_samples, deltas, ridx, pack_infos


def occgrid_raymarch(occ_grid, rays_o, rays_d, near: Union[torch.Tensor, float], far: Union[torch.Tensor, float], *,
                     constraction: Literal['aabb', 'tanh', 'sphere'] = 'aabb', perturb=False,
                     perturb_before_march=False, roi: torch.Tensor = None, step_size: float = 1e-3,
                     max_step_size: float = 1e10, dt_gamma: float = 0.0, max_steps: int = 512,
                     step_size_factor=1.0) -> RaymarchRetSingle:
    """March ``rays_o + t * rays_d`` for t in [near, far) through ``occ_grid`` (bool [Rx, Ry, Rz] over ``roi``,
    default [-1,1]^3), emitting one sample per step inside occupied voxels and skipping empty voxels."""
    step_size, dt_gamma = step_size * step_size_factor, dt_gamma * step_size_factor
    near, far = _as_depth(near, rays_o), _as_depth(far, rays_o)
    if roi is None:
        roi = torch.tensor([-1, -1, -1, 1, 1, 1], dtype=rays_o.dtype, device=rays_o.device)
    ctype = _contraction(constraction)
    if perturb and perturb_before_march:
        near = near + step_size * torch.rand_like(near)
    if FUSED_FINISH and not (perturb and not perturb_before_march) and rays_o.dtype == torch.float32:
        # no jitter after the march: the whole post-processing is two kernels behind the marcher (one readback in all)
        m = _backend.ray_marching_finished(rays_o.contiguous(), rays_d.contiguous(), near.contiguous(), far.contiguous(),
                                           roi.contiguous(), occ_grid.contiguous(), ctype, step_size, max_step_size, dt_gamma,
                                           max_steps, True)
        if m['n_hit'] == 0:
            return RaymarchRetSingle(0, None, None, None, None, None, None, None, None)
        return RaymarchRetSingle(m['n_hit'], m['ridx_hit'], m['samples'], m['t_starts'], m['deltas'], m['ridx'],
                                 m['pack_infos'], m['gidx'].long(), None)
    pack_infos, t_starts, t_ends, ridx, gidx = _backend.ray_marching(
        rays_o.contiguous(), rays_d.contiguous(), near.contiguous(), far.contiguous(), roi.contiguous(),
        occ_grid.contiguous(), ctype, step_size, max_step_size, dt_gamma, max_steps, True)
    out = _finish(rays_o, rays_d, pack_infos, t_starts, t_ends, ridx, perturb and not perturb_before_march)
    if out is None:
        return RaymarchRetSingle(0, None, None, None, None, None, None, None, None)
    ridx_hit, samples, t_starts, _t_samples, deltas, ridx, pack_infos = out
    return RaymarchRetSingle(ridx_hit.numel(), ridx_hit, samples, t_starts, deltas, ridx, pack_infos, gidx.long(), None)


def occgrid_raymarch_batched(occ_grid, rays_o, rays_d, rays_bidx: torch.Tensor = None,
                             near: Union[torch.Tensor, float] = ..., far: Union[torch.Tensor, float] = ..., *,
                             constraction: Literal['aabb', 'tanh', 'sphere'] = 'aabb', perturb=False,
                             perturb_before_march=False, roi: torch.Tensor = None, step_size: float = 1e-3,
                             max_step_size: float = 1e10, dt_gamma: float = 0.0, max_steps: int = 512,
                             step_size_factor=1.0) -> RaymarchRetBatched:
    """Batched grids [B, Rx, Ry, Rz]: rays are either [B, N, 3] (no ``rays_bidx``) or [N, 3] with a per-ray
    batch index."""
    step_size, dt_gamma = step_size * step_size_factor, dt_gamma * step_size_factor
    assert occ_grid.dim() == 4, "Requires batched occ grid input of shape [B,Nx,Ny,Nz]"
    B = occ_grid.shape[0]
    near, far = _as_depth(near, rays_o), _as_depth(far, rays_o)
    if rays_bidx is None:
        assert rays_o.dim() == 3 and rays_o.shape[0] == B, "When not given rays_bidx, inputs should be batched"
        batch_data_size = rays_o.shape[1]
        rays_o, rays_d = rays_o.flatten(0, -2), rays_d.flatten(0, -2)
        near, far = near.flatten(), far.flatten()
    else:
        assert rays_o.dim() == 2 and [*rays_o.shape[:-1]] == [*rays_bidx.shape], \
            "When given rays_bidx, inputs should have the same size with rays_bidx"
        rays_bidx = rays_bidx.int().contiguous()
        batch_data_size = 0
    if roi is None:
        roi = torch.tensor([-1, -1, -1, 1, 1, 1], dtype=rays_o.dtype, device=rays_o.device).tile(B, 1)
    elif roi.dim() == 1:
        roi = roi.tile(B, 1)
    else:
        assert roi.dim() == 2 and roi.shape[0] == B
    ctype = _contraction(constraction)
    if perturb and perturb_before_march:
        near = near + step_size * torch.rand_like(near)
    pack_infos, t_starts, t_ends, ridx, bidx, gidx = _backend.batched_ray_marching(
        rays_o.contiguous(), rays_d.contiguous(), near.contiguous(), far.contiguous(), rays_bidx, batch_data_size,
        roi.contiguous(), occ_grid.contiguous(), ctype, step_size, max_step_size, dt_gamma, max_steps, True)
    out = _finish(rays_o, rays_d, pack_infos, t_starts, t_ends, ridx, perturb and not perturb_before_march)
    if out is None:
        return RaymarchRetBatched(0, None, None, None, None, None, None, None, None, None)
    ridx_hit, samples, _t_starts, t_samples, deltas, ridx, pack_infos = out
    return RaymarchRetBatched(ridx_hit.numel(), ridx_hit, samples, t_samples, deltas, ridx, pack_infos, bidx.long(),
                              gidx.long(), None)


# True: the time-sliced march runs as two launches of the library (bindings._occ_grid.dynamic_ray_marching: frame lookup, static |
# dynamic probe and the per-sample gathers inside the marcher); False: the reference's chain below (lookup ops -> materialised
# union -> batched march -> gathers), kept for A/B and as the cross-check.  Both return the same bits.  The default follows
# profiles/dynamic_march.json (tools/exp_dynamic_march.py): the fused route is faster in every row.
FUSED_DYNAMIC_MARCH = True


_UNIT_ROI = {}


def _empty_dynamic(batched):
    if batched:
        return RaymarchRetBatchedDynamic(0, None, None, None, None, None, None, None, None, None, None)
    return RaymarchRetDynamic(0, None, None, None, None, None, None, None, None, None)


def occgrid_raymarch_dynamic(occ_grid_dynamic: torch.Tensor, ts_keyframes: torch.Tensor, rays_o, rays_d, rays_ts: torch.Tensor,
                             near: Union[torch.Tensor, float], far: Union[torch.Tensor, float], *,
                             occ_grid_static: torch.Tensor = None, rays_bidx: torch.Tensor = None, num_batches: int = None,
                             perturb=False, perturb_before_march=False, step_size: float = 1e-3, max_step_size: float = 1e10,
                             dt_gamma: float = 0.0, max_steps: int = 512,
                             step_size_factor=1.0) -> Union[RaymarchRetDynamic, RaymarchRetBatchedDynamic]:
    """March timestamped rays through time-sliced occupancy: ``occ_grid_dynamic`` bool [n_slices, Rx, Ry, Rz] over [-1, 1]^3 with
    n_slices = T (no ``rays_bidx``) or num_batches * T (slice = batch * T + frame), ``ts_keyframes`` [T] ascending; every ray
    marches the slice of the keyframe nearest to its ``rays_ts`` (``torch_consecutive_nearest1d``), OR-ed with ``occ_grid_static``
    [Rx, Ry, Rz] when given.  What the reference's accelerators do around ``occgrid_raymarch_batched``
    (occgrid_accel/dynamic.py:117-151, :328-364, batched_dynamic.py:69-110).  A ray whose batch index is negative or >=
    num_batches gets no samples on both routes."""
    step_size, dt_gamma = step_size * step_size_factor, dt_gamma * step_size_factor
    assert occ_grid_dynamic.dim() == 4, "Requires time-sliced occ grid input of shape [n_slices,Nx,Ny,Nz]"
    assert rays_o.dim() == 2 and [*rays_o.shape[:-1]] == [*rays_ts.shape], "rays_ts should have one entry per ray"
    T = len(ts_keyframes)
    batched = rays_bidx is not None
    if batched:
        assert [*rays_bidx.shape] == [*rays_ts.shape], "rays_bidx should have one entry per ray"
        if num_batches is None:
            num_batches = occ_grid_dynamic.shape[0] // T
    assert occ_grid_dynamic.shape[0] == (num_batches if batched else 1) * T, "occ_grid_dynamic: one slice per (batch, keyframe)"
    near, far = _as_depth(near, rays_o), _as_depth(far, rays_o)
    perturb_after = perturb and not perturb_before_march
    if perturb and perturb_before_march:
        near = near + step_size * torch.rand_like(near)
    fused = FUSED_DYNAMIC_MARCH and rays_o.is_cuda and rays_o.dtype == torch.float32 and ts_keyframes.dtype == torch.float32 \
        and _backend.dynamic_cache_fits(rays_o.shape[0], max_steps)
    if fused:
        roi = _UNIT_ROI.get(rays_o.device)
        if roi is None:         # one host-to-device copy per device, not per march
            roi = _UNIT_ROI[rays_o.device] = torch.tensor([-1, -1, -1, 1, 1, 1], dtype=torch.float32, device=rays_o.device)
        m = _backend.dynamic_ray_marching(
            rays_o.contiguous(), rays_d.contiguous(), near.contiguous(), far.contiguous(), rays_ts.float().contiguous(), roi,
            occ_grid_dynamic.contiguous(), ts_keyframes.contiguous(), step_size, max_step_size, dt_gamma, max_steps, True,
            grid_static=None if occ_grid_static is None else occ_grid_static.contiguous(),
            batch_inds=rays_bidx.int().contiguous() if batched else None, n_batches=num_batches if batched else 0)
        if m['n_hit'] == 0:
            return _empty_dynamic(batched)
        t_samples, deltas = m['t_starts'], m['deltas']
        if perturb_after:
            # the reference's jitter ops (occgrid_raymarch.py:206-209) on the fused march's outputs
            t_samples = torch.addcmul(m['t_starts'], torch.rand_like(deltas), deltas)
            deltas = packed_diff(t_samples, m['pack_infos'])
        if batched:
            return RaymarchRetBatchedDynamic(m['n_hit'], m['ridx_hit'], m['samples'], t_samples, deltas, m['ridx'], m['pack_infos'],
                                             m['bidx'], m['ts'], m['gidx'].long(), None)
        return RaymarchRetDynamic(m['n_hit'], m['ridx_hit'], m['samples'], t_samples, deltas, m['ridx'], m['pack_infos'], m['ts'],
                                  m['gidx'].long(), None)
    # ---- the chain
    rays_fidx = _nearest1d_torch(ts_keyframes, rays_ts)[0]
    occ_grid = occ_grid_dynamic
    if occ_grid_static is not None:
        if batched:
            occ_grid = (occ_grid_dynamic.unflatten(0, (num_batches, T)) | occ_grid_static).flatten(0, 1)
        else:
            occ_grid = occ_grid_dynamic | occ_grid_static.unsqueeze(0).expand_as(occ_grid_dynamic)
    if batched:
        rays_bidx = rays_bidx.long()
        # (the reference indexes whatever it is given; a raw kernel must not read past the grid)
        rays_flat = torch.where((rays_bidx < 0) | (rays_bidx >= num_batches), -1, rays_bidx * T + rays_fidx)
    else:
        rays_flat = rays_fidx
    ret = occgrid_raymarch_batched(occ_grid, rays_o, rays_d, rays_flat, near, far, perturb=perturb_after, step_size=step_size,
                                   max_step_size=max_step_size, dt_gamma=dt_gamma, max_steps=max_steps)
    if ret.num_hit_rays == 0:
        return _empty_dynamic(batched)
    if batched:
        ret_bi = torch.div(ret.bidx, T, rounding_mode='floor').long()
        ret_ts = ts_keyframes[ret.bidx - ret_bi * T]
        return RaymarchRetBatchedDynamic(ret.num_hit_rays, ret.ridx_hit, ret.samples, ret.depth_samples, ret.deltas, ret.ridx,
                                         ret.pack_infos, ret_bi, ret_ts, ret.gidx, ret.gidx_pack_infos)
    return RaymarchRetDynamic(ret.num_hit_rays, ret.ridx_hit, ret.samples, ret.depth_samples, ret.deltas, ret.ridx, ret.pack_infos,
                              ts_keyframes[ret.bidx], ret.gidx, ret.gidx_pack_infos)


def occgrid_raymarch_forest(forest_meta, occ_grid: torch.Tensor, rays_o, rays_d, near: Union[torch.Tensor, float],
                            far: Union[torch.Tensor, float], seg_block_inds: torch.Tensor, seg_entries: torch.Tensor,
                            seg_exits: torch.Tensor, seg_pack_infos: torch.Tensor, *, perturb=False,
                            perturb_before_march=False, step_size: float = 1e-3, max_step_size: float = 1e10,
                            dt_gamma: float = 0.0, max_steps: int = 512, step_size_factor=1.0) -> RaymarchRetForest:
    """March world-space rays through the per-block grids ``occ_grid`` [n_trees, Rx, Ry, Rz] of a forest, along the
    (block, entry, exit) segments of every ray (``ForestBlockSpace.ray_test``); samples carry their block index
    (occgrid_raymarch.py:223-272)."""
    step_size, dt_gamma = step_size * step_size_factor, dt_gamma * step_size_factor
    near, far = _as_depth(near, rays_o), _as_depth(far, rays_o)
    if perturb and perturb_before_march:
        near = near + step_size * torch.rand_like(near)
    pack_infos, t_starts, t_ends, ridx, blidx, _ = _backend.forest_ray_marching(
        forest_meta, rays_o.contiguous(), rays_d.contiguous(), near.contiguous(), far.contiguous(),
        seg_block_inds.int().contiguous(), seg_entries.contiguous(), seg_exits.contiguous(), seg_pack_infos.int().contiguous(),
        occ_grid.contiguous(), step_size, max_step_size, dt_gamma, max_steps, False)
    out = _finish(rays_o, rays_d, pack_infos, t_starts, t_ends, ridx, perturb and not perturb_before_march)
    if out is None:
        return RaymarchRetForest(0, None, None, None, None, None, None, None, None, None, None)
    ridx_hit, samples, _t_starts, t_samples, deltas, ridx, pack_infos = out
    blidx = blidx.long()
    blidx_pack_infos = get_pack_infos_from_boundary(mark_pack_boundaries(blidx))
    return RaymarchRetForest(ridx_hit.numel(), ridx_hit, samples, t_samples, deltas, ridx, pack_infos, blidx,
                             blidx_pack_infos, None, None)
