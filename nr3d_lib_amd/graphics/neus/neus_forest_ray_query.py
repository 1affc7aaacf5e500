"""NeuS ray queries on a forest of blocks -- counterparts of the three ``_forest_ray_query_inblock_*`` methods of
``NeuSRendererMixinForest`` (nr3d_lib/models/fields_forest/neus/renderer_mixin.py:133-732), as functions of the model:
``neus_forest_ray_query_coarse_multi_upsample`` (:133-272), ``neus_forest_ray_query_march_occ_multi_upsample`` (:274-474) and
``neus_forest_ray_query_march_occ_multi_upsample_compressed`` (:476-732).  Same keywords, defaults, volume-buffer shapes and
``details`` keys.  ``ray_tested`` is what ``ForestBlockSpace.ray_test`` returns (the rays and their packed block segments).

Model protocol: ``space`` (ForestBlockSpace), ``accel`` (OccGridAccelForest; the march-occ pair), ``forward_sdf(x, block_inds)``,
``forward(x, v, block_inds, h_appear=, nablas_has_grad=, with_rgb=, with_normal=)``, ``forward_inv_s()``, ``use_view_dirs``,
``upsample_s_divisor`` (1 when absent).

What sets the forest apart from the single-block drivers of ``neus_ray_query``: every sample carries the index of the block it is
evaluated in.  A new depth inherits the block of the CDF bin it was drawn from, the block indices are merged along with the
depths, and every SDF query takes ``(x, block_inds)``.  The multi-factor loops -- the march-occ pair's and 'multistep_estimate'
of the coarse driver -- are ``_packed_upsample.upsample_loop``, the loop of the single-block drivers, given the block indices as
labels.  While ``FUSED_UPSAMPLE_FOREST`` is set it runs one launch of ``bindings._neus_upsample.upsample_stage_packed_blocks`` per
factor for float32 samples on the GPU; otherwise, and for every other input, the reference's pack-op chain.

Against the reference: ``space.ray_step_coarse`` returns a dict here and the drivers use its keys; the one-factor branch of the
march-occ pair takes ``blidxs_1[0]`` where the reference has ``depths_1[0]`` (:377, :579); the final ``forward`` of the march-occ
pair passes ``block_inds=None`` as the reference does on purpose (the mid-points come from a difference of depths and may have
left the block)."""
from types import SimpleNamespace
from typing import Dict, List, Tuple

import torch

from nr3d_lib_amd.graphics._ray_query import _chunked
from nr3d_lib_amd.graphics.neus._packed_upsample import union, upsample_loop
from nr3d_lib_amd.graphics.neus.neus_utils import neus_packed_sdf_to_alpha, neus_ray_sdf_to_alpha
from nr3d_lib_amd.graphics.pack_ops import (get_pack_infos_from_batch, merge_two_packs_sorted_a_includes_b, packed_diff,
                                            packed_volume_render_compression)
from nr3d_lib_amd.profile import profile

__all__ = ['neus_forest_ray_query_coarse_multi_upsample', 'neus_forest_ray_query_march_occ_multi_upsample',
           'neus_forest_ray_query_march_occ_multi_upsample_compressed']

# One up-sampling stage of the loop (read at call time and handed to it as `fused`): True = one launch of the block-carrying packed
# HIP kernel per factor for float32 samples on the GPU, no union on the last factor; False (and every other input) = the reference's
# pack-op chain.  Same semantics.
# Measured (profiles/neus_forest_query.json, tools/exp_neus_forest_query.py): the fused route's median is below the chain's in every row.
FUSED_UPSAMPLE_FOREST = True

_SEG_KEYS = ('seg_block_inds', 'seg_entries', 'seg_exits', 'seg_pack_infos')


def _setup(model, ray_tested, forward_inv_s, upsample_inv_s, with_rgb, with_normal, nablas_has_grad) -> SimpleNamespace:
    """what the three drivers share: the ray tensors, the model's switches, and the two model queries"""
    q = SimpleNamespace(model=model, ray_tested=ray_tested)
    q.upsample_inv_s = upsample_inv_s / getattr(model, 'upsample_s_divisor', 1.0)
    q.forward_inv_s = model.forward_inv_s() if forward_inv_s is None else forward_inv_s
    q.rays_o, q.rays_d, q.near, q.far, q.rays_inds = (ray_tested[k] for k in ('rays_o', 'rays_d', 'near', 'far', 'rays_inds'))
    assert q.rays_o.dim() == 2 and q.rays_d.dim() == 2
    q.device, q.dtype = q.rays_o.device, q.rays_o.dtype
    q.segs = tuple(ray_tested[k] for k in _SEG_KEYS)
    # the normalised ray direction in the network's space (rays_d may carry a scale)
    q.view_dirs = q.rays_d / q.rays_d.data.norm(dim=-1).clamp_min_(1.0e-10).unsqueeze(-1)
    use_view_dirs, h_appear = bool(getattr(model, 'use_view_dirs', False)), ray_tested.get('rays_h_appear', None)

    def step_coarse(**cfg):
        return model.space.ray_step_coarse(q.rays_o, q.rays_d, q.near, q.far, *q.segs, **cfg)

    def sdf(x, block_inds, chunk=None):
        """forward_sdf; in slices of `chunk` rows unless the model is training"""
        if chunk is None or getattr(model, 'training', False):
            return model.forward_sdf(x, block_inds)['sdf']
        return _chunked(lambda x, block_inds: model.forward_sdf(x, block_inds)['sdf'], dict(x=x, block_inds=block_inds), chunk)

    def net(vb, x, pick, block_inds):
        """the full query at x; `pick` maps a per-ray tensor to x's layout.  Adds 'nablas' / 'rgb' to the volume buffer"""
        if not (with_rgb or with_normal):
            return vb
        out = model.forward(x, pick(q.view_dirs) if use_view_dirs else None, block_inds,
                            h_appear=None if h_appear is None else pick(h_appear),
                            nablas_has_grad=nablas_has_grad, with_rgb=with_rgb, with_normal=with_normal)
        for k in ('nablas', 'rgb'):
            if k in out:
                vb[k] = out[k].to(q.dtype)
        return vb

    q.step_coarse, q.sdf, q.net = step_coarse, sdf, net
    q.pts = lambda ridx, t: torch.addcmul(q.rays_o[ridx], q.rays_d[ridx], t.unsqueeze(-1))
    return q


def _upsample_loop(q, hit, depth, sdf, blidx, pack_infos, num_fine, factors, use_estimate_alpha, perturb):
    """``_packed_upsample.upsample_loop`` on the packs of the rays `hit`, every sample with its block index: ``num_fine`` new depths per
    factor, ``model.forward_sdf(x_fine, blidx_fine)`` between factors"""
    return upsample_loop(q.rays_o[hit], q.rays_d[hit], depth, sdf, pack_infos, blidx, [num_fine] * len(factors), factors, q.upsample_inv_s,
                         use_estimate_alpha, perturb, FUSED_UPSAMPLE_FOREST,
                         lambda x, blidx_fine: q.sdf(x.flatten(0, -2), blidx_fine.flatten()))


def _one_stage(q, ret, num_fine, use_estimate_alpha, perturb, chunk=None):
    """'direct_use' / 'direct_more': one stage of ``num_fine`` new depths on the stepped samples `ret`, joined to them
    -> (depth, blidx, pack_infos, the ray of every pack)"""
    sdf = q.sdf(ret['samples'], ret['blidx'], chunk)
    fines, blidx_fines, _ = _upsample_loop(q, ret['ridx_hit'], ret['depth_samples'], sdf, ret['blidx'], ret['pack_infos'], num_fine, [1],
                                           use_estimate_alpha, perturb)
    return (*union(ret['depth_samples'], ret['blidx'], ret['pack_infos'], fines[0], blidx_fines[0])[:3], ret['ridx_hit'])


def neus_forest_ray_query_coarse_multi_upsample(
        model, ray_tested: Dict[str, torch.Tensor],
        with_rgb: bool = True, with_normal: bool = True, perturb: bool = False, nablas_has_grad: bool = False,
        forward_inv_s: float = None,
        coarse_step_cfg=dict(), step_size_nograd: float = 0.01, chunksize_query: int = 2 ** 24,
        upsample_mode: str = 'direct_more', num_fine: int = 64, upsample_inv_s: float = 64.,
        upsample_inv_s_factors: List[int] = [1, 4, 16], upsample_use_estimate_alpha=False) -> Tuple[dict, dict]:
    """Coarse steps inside the block segments of every ray, up-sampled without gradient, then ``forward_sdf`` at all depths for the
    opacities and ``forward`` at the interval mid-points: always a packed buffer over all tested rays.
    ``upsample_mode``: 'direct_use' -- one stage of ``num_fine`` on the coarse samples; 'direct_more' -- one stage of ``num_fine`` on
    linear steps of ``step_size_nograd`` (``ray_step_coarse(step_mode='linear')``, queried in chunks), joined to those;
    'multistep_estimate' -- ``num_fine // 2 * 2 + 1`` new depths per entry of ``upsample_inv_s_factors`` on the coarse samples (with
    one entry the reference joins nothing and the buffer holds the coarse samples; kept)."""
    if ray_tested['num_rays'] == 0:
        return dict(type='empty'), {}
    q = _setup(model, ray_tested, forward_inv_s, upsample_inv_s, with_rgb, with_normal, nablas_has_grad)
    coarse = q.step_coarse(**coarse_step_cfg)

    @torch.no_grad()
    def upsample():
        if upsample_mode == 'direct_use':
            return _one_stage(q, coarse, num_fine, upsample_use_estimate_alpha, perturb)
        if upsample_mode == 'direct_more':
            more = q.step_coarse(step_mode='linear', step_size=step_size_nograd, max_steps=4096, perturb=perturb)
            return _one_stage(q, more, num_fine, upsample_use_estimate_alpha, perturb, chunksize_query)
        if upsample_mode == 'multistep_estimate':
            hit = coarse['ridx_hit']
            fines, blidx_fines, state = _upsample_loop(
                q, hit, coarse['depth_samples'], q.sdf(coarse['samples'], coarse['blidx']), coarse['blidx'], coarse['pack_infos'],
                num_fine // 2 * 2 + 1, upsample_inv_s_factors, upsample_use_estimate_alpha, perturb)
            if len(upsample_inv_s_factors) > 1:
                return (*union(*state, fines[-1], blidx_fines[-1])[:3], hit)
            return (*state, hit)
        raise RuntimeError(f"Invalid upsample_mode={upsample_mode}")

    with profile("Upsampling"):
        d_all, blidx_all, pack_infos, ridx_packs = upsample()         # the ray of every pack: from the steps that were up-sampled
    with profile("Acquire volume buffer"):
        ridx_all = torch.repeat_interleave(ridx_packs, pack_infos[:, 1], output_size=d_all.numel())
        d_mid = d_all + packed_diff(d_all, pack_infos) / 2.
        alpha = neus_packed_sdf_to_alpha(q.sdf(q.pts(ridx_all, d_all), blidx_all), q.forward_inv_s, pack_infos)
        # (every stepper gives every tested ray a pack, min_steps at the least: the packs are the tested rays, as in the reference)
        vb = dict(type='packed', rays_inds_hit=q.rays_inds, pack_infos_hit=pack_infos, t=d_mid.to(q.dtype),
                  opacity_alpha=alpha.to(q.dtype))
        q.net(vb, q.pts(ridx_all, d_mid), lambda t: t[ridx_all], blidx_all)
    return vb, {'render.num_per_ray': pack_infos[:, 1]}


def _march_and_upsample(q, perturb, coarse_step_cfg, chunksize_query, march_cfg, num_fine, factors, use_estimate_alpha):
    """the front half of the march-occ pair -> (coarse steps | None, the marcher's record, and for hit rays the new depths
    [num_hit, len(factors) m] sorted per ray with their block indices, m = num_fine // 2 * 2 + 1)"""
    model = q.model
    assert getattr(model, 'accel', None) is not None, "Need a non-empty AccelStruct"
    coarse = q.step_coarse(**coarse_step_cfg) if coarse_step_cfg is not None else None
    with profile("Ray marching"):
        marched = model.accel.ray_march(q.rays_o, q.rays_d, q.near, q.far, *q.segs, perturb=perturb, **march_cfg)
    if marched.ridx_hit is None:
        return coarse, marched, None, None
    with profile("Upsampling"), torch.no_grad():
        hit = marched.ridx_hit
        sdf = _chunked(lambda x, block_inds: model.forward_sdf(x, block_inds)['sdf'],
                       dict(x=marched.samples, block_inds=marched.blidx), chunksize_query)
        fines, blidx_fines, _ = _upsample_loop(q, hit, marched.depth_samples, sdf, marched.blidx, marched.pack_infos.clone(),
                                               num_fine // 2 * 2 + 1, factors, use_estimate_alpha, perturb)
        if len(factors) > 1:
            depths_1, order = torch.cat(fines, dim=-1).sort(dim=-1)
            blidxs_1 = torch.cat(blidx_fines, dim=-1).gather(-1, order)
        else:
            depths_1, blidxs_1 = fines[0], blidx_fines[0]
    return coarse, marched, depths_1, blidxs_1


def _join_coarse(coarse, hit, depths_1, blidxs_1):
    """coarse steps of every ray + the new depths of the hit rays, sorted per ray -> (ridx, blidx, depth, pack_infos), packed"""
    pinfo_fine = get_pack_infos_from_batch(hit.numel(), depths_1.shape[-1], device=depths_1.device)
    pidx0, pidx1, pack_infos = merge_two_packs_sorted_a_includes_b(
        coarse['depth_samples'], coarse['pack_infos'], coarse['ridx_hit'], depths_1.flatten(), pinfo_fine, hit, b_sorted=True,
        return_val=False)
    total = depths_1.numel() + coarse['depth_samples'].numel()
    depth, ridx, blidx = depths_1.new_zeros([total]), hit.new_zeros([total]), blidxs_1.new_zeros([total])
    ridx[pidx0], ridx[pidx1] = coarse['ridx'], hit.unsqueeze(-1).expand(-1, depths_1.shape[-1]).flatten()
    blidx[pidx0], blidx[pidx1] = coarse['blidx'], blidxs_1.flatten()
    depth[pidx0], depth[pidx1] = coarse['depth_samples'], depths_1.flatten()
    return ridx, blidx, depth, pack_infos


def neus_forest_ray_query_march_occ_multi_upsample(
        model, ray_tested: Dict[str, torch.Tensor],
        with_rgb: bool = True, with_normal: bool = True, perturb: bool = False, nablas_has_grad: bool = False,
        forward_inv_s: float = None,
        coarse_step_cfg: dict = None, chunksize_query: int = 2 ** 24, march_cfg=dict(), num_fine: int = 8,
        upsample_inv_s: float = 64., upsample_inv_s_factors: List[int] = [1, 4, 16],
        upsample_use_estimate_alpha=False) -> Tuple[dict, dict]:
    """Rays marched through the per-block occupancy grids, the marched samples up-sampled once per entry of
    ``upsample_inv_s_factors``.  Result: a batched buffer of the new depths' mid-points on the hit rays (``coarse_step_cfg`` None); a
    packed buffer of coarse steps and new depths over all tested rays; the packed coarse steps alone when nothing is marched; empty."""
    empty = dict(type='empty', rays_inds_hit=[])
    if ray_tested['num_rays'] == 0:
        return empty, {}
    q = _setup(model, ray_tested, forward_inv_s, upsample_inv_s, with_rgb, with_normal, nablas_has_grad)
    coarse, marched, depths_1, blidxs_1 = _march_and_upsample(q, perturb, coarse_step_cfg, chunksize_query, march_cfg, num_fine,
                                                              upsample_inv_s_factors, upsample_use_estimate_alpha)
    hit, dtype = marched.ridx_hit, q.dtype
    with profile("Acquire volume buffer"):
        if hit is None:
            if coarse is None:
                return empty, {}
            alpha = neus_packed_sdf_to_alpha(q.sdf(coarse['samples'], coarse['blidx']), q.forward_inv_s, coarse['pack_infos'])
            depths = coarse['depth_samples'] + coarse['deltas'] / 2.
            vb = dict(type='packed', rays_inds_hit=q.rays_inds[coarse['ridx_hit']], pack_infos_hit=coarse['pack_infos'],
                      t=depths.to(dtype), opacity_alpha=alpha.to(dtype))
            q.net(vb, q.pts(coarse['ridx'], depths), lambda t: t[coarse['ridx']], coarse['blidx'])
            return vb, {'render.num_per_ray': coarse['pack_infos'][:, 1]}

        details = {'march.num_per_ray': marched.pack_infos[:, 1]}
        if coarse is None:
            o_hit, d_hit = q.rays_o[hit].unsqueeze(-2), q.rays_d[hit].unsqueeze(-2)
            alpha = neus_ray_sdf_to_alpha(q.sdf(torch.addcmul(o_hit, d_hit, depths_1.unsqueeze(-1)), blidxs_1), q.forward_inv_s)
            depths = depths_1[..., :-1] + depths_1.diff(dim=-1) / 2.
            vb = dict(type='batched', rays_inds_hit=q.rays_inds[hit], num_per_hit=depths.shape[-1], t=depths.to(dtype),
                      opacity_alpha=alpha.to(dtype))
            q.net(vb, torch.addcmul(o_hit, d_hit, depths.unsqueeze(-1)), lambda t: t[hit].unsqueeze(-2), None)
            details['render.num_per_ray'] = depths.shape[-1]
            return vb, details

        ridx_all, blidx_all, depths_1p, pack_infos = _join_coarse(coarse, hit, depths_1, blidxs_1)
        alpha = neus_packed_sdf_to_alpha(q.sdf(q.pts(ridx_all, depths_1p), blidx_all), q.forward_inv_s, pack_infos)
        depths = depths_1p + packed_diff(depths_1p, pack_infos) / 2.
        vb = dict(type='packed', rays_inds_hit=q.rays_inds, pack_infos_hit=pack_infos, t=depths.to(dtype),
                  opacity_alpha=alpha.to(dtype))
        q.net(vb, q.pts(ridx_all, depths), lambda t: t[ridx_all], None)
        details['render.num_per_ray'] = pack_infos[:, 1]
        return vb, details


def neus_forest_ray_query_march_occ_multi_upsample_compressed(
        model, ray_tested: Dict[str, torch.Tensor],
        with_rgb: bool = True, with_normal: bool = True, perturb: bool = False, nablas_has_grad: bool = False,
        forward_inv_s: float = None,
        coarse_step_cfg: dict = None, chunksize_query: int = 2 ** 24, march_cfg=dict(), num_fine: int = 8,
        upsample_inv_s: float = 64., upsample_inv_s_factors: List[int] = [1, 4, 16],
        upsample_use_estimate_alpha=False) -> Tuple[dict, dict]:
    """The same up-sampling, then ``packed_volume_render_compression`` on the opacities of the final samples: always a packed buffer
    over the rays that keep a sample, and only the kept samples reach ``model.forward``.  The SDF of the final samples is queried in
    chunks of ``chunksize_query`` unless the model is training."""
    empty = dict(type='empty', rays_inds_hit=[])
    if ray_tested['num_rays'] == 0:
        return empty, {}
    q = _setup(model, ray_tested, forward_inv_s, upsample_inv_s, with_rgb, with_normal, nablas_has_grad)
    coarse, marched, depths_1, blidxs_1 = _march_and_upsample(q, perturb, coarse_step_cfg, chunksize_query, march_cfg, num_fine,
                                                              upsample_inv_s_factors, upsample_use_estimate_alpha)
    hit, dtype = marched.ridx_hit, q.dtype

    def compressed_buffer(alpha, depths, ridx, blidx, pack_infos, rays_of_packs, details):
        """alpha / depths / ridx / blidx (None: the forest finds the block): flat per sample, packs described by pack_infos"""
        nidx_useful, pack_infos_useful, pidx_useful = packed_volume_render_compression(alpha, pack_infos)
        if nidx_useful.numel() == 0:
            return empty, {}
        depths, alpha, ridx = depths[pidx_useful], alpha[pidx_useful], ridx[pidx_useful]
        vb = dict(type='packed', rays_inds_hit=rays_of_packs[nidx_useful], pack_infos_hit=pack_infos_useful, t=depths.to(dtype),
                  opacity_alpha=alpha.to(dtype))
        q.net(vb, q.pts(ridx, depths), lambda t: t[ridx], None if blidx is None else blidx[pidx_useful])
        details['render.num_per_ray'] = pack_infos_useful[:, 1]
        return vb, details

    with profile("Acquire volume buffer"):
        if hit is None:
            if coarse is None:
                return empty, {}
            alpha = neus_packed_sdf_to_alpha(q.sdf(coarse['samples'], coarse['blidx'], chunksize_query), q.forward_inv_s,
                                             coarse['pack_infos'])
            return compressed_buffer(alpha, coarse['depth_samples'] + coarse['deltas'] / 2., coarse['ridx'], coarse['blidx'],
                                     coarse['pack_infos'], q.rays_inds[coarse['ridx_hit']],
                                     {'render.num_per_ray0': coarse['pack_infos'][:, 1]})

        details = {'march.num_per_ray': marched.pack_infos[:, 1]}
        if coarse is None:
            o_hit, d_hit = q.rays_o[hit].unsqueeze(-2), q.rays_d[hit].unsqueeze(-2)
            alpha = neus_ray_sdf_to_alpha(q.sdf(torch.addcmul(o_hit, d_hit, depths_1.unsqueeze(-1)), blidxs_1, chunksize_query),
                                          q.forward_inv_s)
            depths = depths_1[..., :-1] + depths_1.diff(dim=-1) / 2.
            details['render.num_per_ray0'] = depths.shape[-1]
            return compressed_buffer(alpha.flatten(), depths.flatten(), hit.unsqueeze(-1).expand(-1, depths.shape[-1]).flatten(), None,
                                     get_pack_infos_from_batch(hit.numel(), depths.shape[-1], device=q.device), q.rays_inds[hit],
                                     details)

        ridx_all, blidx_all, depths_1p, pack_infos = _join_coarse(coarse, hit, depths_1, blidxs_1)
        depths = depths_1p + packed_diff(depths_1p, pack_infos) / 2.
        alpha = neus_packed_sdf_to_alpha(q.sdf(q.pts(ridx_all, depths_1p), blidx_all, chunksize_query), q.forward_inv_s, pack_infos)
        details['render.num_per_ray0'] = pack_infos[:, 1]
        return compressed_buffer(alpha, depths, ridx_all, None, pack_infos, q.rays_inds, details)
