"""NeuS ray query with multi-stage up-sampling on occupancy-grid marched samples (StreetSurf sec. 4.1).

Counterpart of ``neus_ray_query_march_occ_multi_upsample`` (nr3d_lib/graphics/neus/neus_ray_query.py:358-729): same
signature, ``ray_tested`` keys, model protocol (``forward``, ``forward_sdf``, ``forward_inv_s``, ``accel``; the
``use_*`` / ``fwd_sdf_use_*`` attribute flags) and the four result shapes -- batched buffer of the fine samples
(``num_coarse == 0``), packed buffer of coarse + fine samples, batched coarse-only buffer when nothing is hit, empty.
The up-sampling loop is where the secondary pack ops run end to end on the device: SDF at the marched samples ->
opacity -> ``packed_alpha_to_vw`` -> exclusive ``packed_cumsum`` normalised with ``packed_div`` -> ``packed_sample_cdf``
(``packed_invert_cdf``) -> ``merge_two_packs_sorted_aligned`` of the new depths into the packed buffer, once per
``upsample_inv_s_factors`` entry; ``merge_two_batch_a_includes_b`` joins coarse and fine samples.
(The reference reads ``marched.ridx_hitx`` at :470, an attribute its records do not have; ``ridx_hit`` is used here.)

``neus_ray_query_coarse_multi_upsample`` (:132-356) is the vanilla NeuS query that needs no occupancy grid: coarse boundaries on
every ray between ``near`` and ``far``, the up-sampling on fixed-length rows, one query at the mid-points.  Its stage runs in one
launch (``bindings._neus_upsample.upsample_stage``) while ``FUSED_UPSAMPLE`` is set.  The stage of the march-occ drivers runs in
one launch on the packs (``upsample_stage_packed``) while ``FUSED_UPSAMPLE_PACKED`` is set, in place of the pack-op chain above;
the loop itself is ``_packed_upsample.upsample_loop``, which the forest drivers of ``neus_forest_ray_query`` share.
The opacity of the final samples (``neus_ray_sdf_to_alpha`` / ``neus_packed_sdf_to_alpha``) is one launch each way while
``neus_utils.FUSED_SDF_TO_ALPHA`` is set; the op chains of the two switches above, when off, pass ``fused=False``."""
from types import SimpleNamespace
from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

from nr3d_lib_amd.bindings import _neus_upsample
from nr3d_lib_amd.graphics._ray_query import _chunked, _flag, _march
from nr3d_lib_amd.graphics.nerf.nerf_utils import ray_alpha_to_vw
from nr3d_lib_amd.graphics.neus._packed_upsample import upsample_loop
from nr3d_lib_amd.graphics.neus.neus_utils import neus_packed_sdf_to_alpha, neus_ray_sdf_to_alpha, neus_ray_sdf_to_upsample_alpha
from nr3d_lib_amd.graphics.pack_ops import (get_pack_infos_from_batch, merge_two_batch_a_includes_b, packed_diff,
                                            packed_volume_render_compression)
from nr3d_lib_amd.graphics.raysample import (batch_sample_pdf, batch_sample_step_linear, batch_sample_step_wrt_depth,
                                             batch_sample_step_wrt_sqrt_depth, cdf_positions)
from nr3d_lib_amd.profile import profile

__all__ = ['neus_ray_query_sphere_trace', 'neus_ray_query_coarse_multi_upsample', 'neus_ray_query_march_occ_multi_upsample',
           'neus_ray_query_march_occ_multi_upsample_compressed', 'neus_ray_query_march_occ_multi_upsample_compressed_strategy']

# The stage of neus_ray_query_coarse_multi_upsample between two SDF queries: True = one launch of the HIP kernel for rows that are
# float32, on the GPU and within _neus_upsample.MAX_ROW; False (and every other row) = the reference's torch op chain.  Same semantics.
FUSED_UPSAMPLE = True
# The stage of the march-occ drivers (read at call time and handed to _packed_upsample.upsample_loop as `fused`): True = one launch of the
# packed HIP kernel per stage for float32 samples on the GPU, no merge on the last stage; False (and every other input) = the
# reference's pack-op chain.  Same semantics.
FUSED_UPSAMPLE_PACKED = True

_RAY_ATTRS = (('ts', 'rays_ts'), ('fidx', 'rays_fidx'), ('bidx', 'rays_bidx'), ('pix', 'rays_pix'),
              ('h_appear', 'rays_h_appear'))
_COARSE_SAMPLERS = dict(linear=batch_sample_step_linear, depth=batch_sample_step_wrt_depth,
                        sqrt_depth=batch_sample_step_wrt_sqrt_depth)


def _check_model(model, need_accel=True):
    for need in ('forward', 'forward_sdf', 'forward_inv_s'):
        assert hasattr(model, need), f"model.{need}() is requried"
    assert not need_accel or getattr(model, 'accel', None) is not None, "model.accel is required"


class _Query(SimpleNamespace):
    """what both drivers share: the model's attribute protocol resolved once, the ray tensors, and the two model queries"""


def _setup(model, ray_tested, with_rgb, with_normal, nablas_has_grad, forward_inv_s, num_fine, upsample_inv_s,
           upsample_s_divisor, upsample_inv_s_factors) -> _Query:
    q = _Query(model=model, ray_tested=ray_tested, with_rgb=with_rgb, with_normal=with_normal)
    q.sdf_uses = {k: _flag(model, 'use_' + k) if k in ('ts', 'fidx', 'bidx') else _flag(model, 'fwd_sdf_use_' + k)
                  for k, _ in _RAY_ATTRS}
    q.full_uses = {k: q.sdf_uses[k] or (_flag(model, 'use_' + k) and with_rgb) for k, _ in _RAY_ATTRS}
    q.sdf_view = _flag(model, 'fwd_sdf_use_view_dirs')
    q.full_view = q.sdf_view or (_flag(model, 'use_view_dirs') and with_rgb)
    q.n_stages = len(upsample_inv_s_factors)
    num_fine = [num_fine] * q.n_stages if isinstance(num_fine, int) else list(num_fine)
    assert len(num_fine) == q.n_stages, f"num_fine should be of the same length={q.n_stages} with upsample"
    q.num_fine = [n // 2 * 2 + 1 for n in num_fine]                     # odd counts: a sample at the median
    q.upsample_inv_s = upsample_inv_s / upsample_s_divisor
    q.forward_inv_s = model.forward_inv_s() if forward_inv_s is None else forward_inv_s
    q.rays_o, q.rays_d = ray_tested['rays_o'], ray_tested['rays_d']
    q.near, q.far, q.rays_inds = ray_tested['near'], ray_tested['far'], ray_tested['rays_inds']
    assert q.rays_o.dim() == 2 and q.rays_d.dim() == 2
    q.device, q.dtype = q.rays_o.device, q.rays_o.dtype
    q.view_dirs = (q.rays_d / q.rays_d.detach().norm(dim=-1, keepdim=True).clamp_min(1.0e-10)) if q.full_view else None

    def attrs(uses, use_view, pick):
        """per-ray extras of the model query; `pick` maps a [num_rays, ...] tensor to the layout of the query points"""
        kw = {k: pick(ray_tested[src]) for k, src in _RAY_ATTRS if uses[k]}
        if use_view:
            kw['v'] = pick(q.view_dirs)
        return kw

    def spread(sel, *shape):
        """pick for points laid out as [len(sel), *shape]: the ray's value repeated over its samples"""
        def pick(t):
            t = t if sel is None else t[sel]
            return t.reshape(t.shape[0], *([1] * len(shape)), *t.shape[1:]).expand(t.shape[0], *shape, *t.shape[1:]).contiguous()
        return pick

    def query_sdf(x, extra):
        return model.forward_sdf(x=x, **extra)['sdf']

    def full_query(x, extra):
        out = model.forward(x=x, nablas_has_grad=nablas_has_grad, with_rgb=with_rgb, with_normal=with_normal, **extra)
        buf = {'net_x': x}
        for k in ('nablas', 'rgb'):
            if k in out:
                buf[k] = out[k].to(q.dtype)
        return buf

    def finish(vb, rays_sel, pts, pick):
        """the last two steps of every volume buffer: ``rays_bidx_hit`` of its rays (`rays_sel` indexes the tested rays, None: all of
        them) and the full query at ``pts()`` with the per-ray extras laid out by `pick`"""
        if q.full_uses['bidx']:
            vb['rays_bidx_hit'] = ray_tested['rays_bidx'] if rays_sel is None else ray_tested['rays_bidx'][rays_sel]
        if with_rgb or with_normal:
            vb.update(full_query(pts(), q.full_attrs(pick)))
        return vb

    q.attrs, q.spread, q.query_sdf, q.full_query, q.finish = attrs, spread, query_sdf, full_query, finish
    q.sdf_attrs = lambda pick: attrs(q.sdf_uses, q.sdf_view, pick)
    q.full_attrs = lambda pick: attrs(q.full_uses, q.full_view, pick)
    return q


def _coarse_boundaries(q, num_coarse, coarse_step_cfg, perturb):
    """num_coarse + 1 interval boundaries per ray and their spacings"""
    cfg = dict(coarse_step_cfg)
    mode = cfg.pop('step_mode')
    if mode not in _COARSE_SAMPLERS:
        raise RuntimeError(f"Invalid step_mode={mode}")
    return _COARSE_SAMPLERS[mode](q.near, q.far, num_coarse + 1, perturb=perturb, return_dt=True, **cfg)


def _sdf_maybe_chunked(q, x, extra, chunksize_query):
    if q.model.training:
        return q.query_sdf(x, extra)
    return _chunked(lambda x, **kw: q.query_sdf(x, kw), dict(x=x, **extra), chunksize_query)


def _march_and_upsample(q, perturb, num_coarse, coarse_step_cfg, chunksize_query, march_cfg, factors, use_estimate_alpha,
                        want_stages=False):
    """the front half of the march-occ pair -> (coarse boundaries [num_rays, num_coarse + 1] and their spacings | None, None, the marcher's
    record, and for hit rays the new depths [num_hit, sum(num_fine)] sorted per ray, with `want_stages` the factor (1-based) each came
    from | None)"""
    depths_coarse_1, deltas_coarse_1 = _coarse_boundaries(q, num_coarse, coarse_step_cfg, perturb) if num_coarse > 0 else (None, None)
    with profile("Ray marching"):
        marched = _march(q.model, q.ray_tested, q.rays_o, q.rays_d, q.near, q.far, perturb, march_cfg)
    if marched.ridx_hit is None:
        return depths_coarse_1, deltas_coarse_1, marched, None, None
    with profile("Upsampling"), torch.no_grad():
        hit = marched.ridx_hit
        sdf = _chunked(lambda x, **kw: q.query_sdf(x, kw),
                       dict(x=marched.samples, **q.sdf_attrs(lambda t: t[marched.ridx])), chunksize_query)

        def sdf_at(x, _):
            extra = {k: v.flatten(0, 1) for k, v in q.sdf_attrs(q.spread(hit, x.shape[1])).items()}
            return q.query_sdf(x.flatten(0, -2), extra)

        fines, _, _ = upsample_loop(q.rays_o[hit], q.rays_d[hit], marched.depth_samples, sdf, marched.pack_infos.clone(), None, q.num_fine,
                                    factors, q.upsample_inv_s, use_estimate_alpha, perturb, FUSED_UPSAMPLE_PACKED, sdf_at)
        depths_1, order = torch.cat(fines, dim=-1).sort(dim=-1) if q.n_stages > 1 else (fines[0], None)
        stages = None
        if want_stages:                                    # only debug_query_data reads them, and repeat_interleave waits for the host
            stage_of = torch.repeat_interleave(1 + torch.arange(q.n_stages, device=q.device), torch.tensor(q.num_fine, device=q.device))
            stages = stage_of.expand_as(depths_1) if order is None else stage_of[order]
    return depths_coarse_1, deltas_coarse_1, marched, depths_1, stages


def _join_coarse(depths_coarse_1, hit, depths_1, stages=None):
    """coarse boundaries of every ray + the new depths of the hit rays, sorted per ray -> (ridx, depth, pack_infos, the factor every
    element came from: 0 for a coarse boundary | None without `stages`), packed over ALL tested rays"""
    all_rays = torch.arange(depths_coarse_1.shape[0], device=depths_1.device)
    pidx0, pidx1, pack_infos = merge_two_batch_a_includes_b(depths_coarse_1, all_rays, depths_1, hit, a_sorted=True)
    total = depths_1.numel() + depths_coarse_1.numel()
    depth, ridx = depths_1.new_zeros(total), hit.new_zeros(total)
    ridx[pidx0], ridx[pidx1] = all_rays.unsqueeze(-1), hit.unsqueeze(-1)
    depth[pidx0], depth[pidx1] = depths_coarse_1, depths_1
    stages_p = None
    if stages is not None:
        stages_p = stages.new_zeros(total)
        stages_p[pidx0], stages_p[pidx1] = 0, stages
    return ridx, depth, pack_infos, stages_p


def _row_stage(depth, sdf, num_fine, inv_s, use_estimate_alpha, perturb):
    """one up-sampling stage on rows depth, sdf [num_rays, n] -> (the num_fine new depths, the sorted union [num_rays, n + num_fine],
    the position in cat([depth, fine], -1) of every element of the union)"""
    if FUSED_UPSAMPLE and depth.is_cuda and depth.dtype == torch.float32 and sdf.dtype == torch.float32 \
            and depth.shape[-1] + num_fine <= _neus_upsample.MAX_ROW:
        u = cdf_positions(depth, depth.shape[:-1], num_fine, perturb)
        return _neus_upsample.upsample_stage(depth.contiguous(), sdf.contiguous(), u, inv_s, use_estimate_alpha)
    # this route stays the reference's op chain (fused=False: no kernel of neus_utils.FUSED_SDF_TO_ALPHA either)
    alpha = neus_ray_sdf_to_upsample_alpha(sdf, depth, inv_s) if use_estimate_alpha else neus_ray_sdf_to_alpha(sdf, inv_s, fused=False)
    fine = batch_sample_pdf(depth, ray_alpha_to_vw(alpha), num_fine, perturb=perturb)
    merged, order = torch.sort(torch.cat([depth, fine], dim=-1), dim=-1)
    return fine, merged, order


def neus_ray_query_coarse_multi_upsample(
        model, ray_tested: Dict[str, torch.Tensor],
        with_rgb: bool = True, with_normal: bool = True, perturb: bool = False, nablas_has_grad: bool = False,
        forward_inv_s: float = None,
        compression=True, num_coarse: int = 64, coarse_step_cfg=dict(step_mode='linear'),
        upsample_mode: str = 'multistep_estimate', num_fine: int = 64,
        upsample_inv_s: float = 64., upsample_s_divisor: float = 1.0,
        upsample_inv_s_factors: List[int] = [1, 2, 4, 8], upsample_use_estimate_alpha=False,
        num_nograd: int = 1024, chunksize_query: int = 2 ** 24) -> Tuple[dict, dict]:
    """Vanilla NeuS ray query (nr3d_lib/graphics/neus/neus_ray_query.py:132-356): ``num_coarse + 1`` boundaries per ray, up-sampled
    without gradient, then ``model.forward_sdf`` at all boundaries for the opacities and ``model.forward`` at the interval mid-points.
    ``upsample_mode``: 'multistep_estimate' -- one stage of ``num_fine // 2 * 2 + 1`` new depths per entry of
    ``upsample_inv_s_factors``, the SDF queried at the new depths between stages; 'direct_use' -- one stage of ``num_fine`` on the
    coarse boundaries; 'direct_more' -- one stage of ``num_fine`` on ``num_nograd`` uniform boundaries (queried in chunks).
    Result: the empty buffer; ``type='batched'`` over all tested rays (``compression=False``); or ``type='packed'`` over the rays
    that keep a sample after ``packed_volume_render_compression`` -- only those samples reach ``model.forward``.
    Two reference defects, neither mode runs there: 'direct_use' and 'direct_more' call ``.sort(d_all, dim=-1)`` on a name that is
    not bound yet (:220, :239) -- a sort along the last axis is meant; 'direct_more' lerps ``near`` [num_rays] against
    [num_nograd] steps without unsqueezing (:222) -- ``near`` / ``far`` are taken as columns."""
    _check_model(model, need_accel=False)
    empty = dict(type='empty', rays_inds_hit=[])
    if ray_tested['num_rays'] == 0:
        return empty, {}
    q = _setup(model, ray_tested, with_rgb, with_normal, nablas_has_grad, forward_inv_s, num_fine, upsample_inv_s,
               upsample_s_divisor, upsample_inv_s_factors)
    rays_o, rays_d, rays_inds, device, dtype = q.rays_o, q.rays_d, q.rays_inds, q.device, q.dtype
    depths_coarse_1, _ = _coarse_boundaries(q, num_coarse, coarse_step_cfg, perturb)
    pts = lambda d: torch.addcmul(rays_o[..., None, :], rays_d[..., None, :], d[..., None])
    sdf_extra = lambda d: q.sdf_attrs(q.spread(None, d.shape[-1]))

    @torch.no_grad()
    def upsample():
        if upsample_mode == 'multistep_estimate':
            d_all = depths_coarse_1
            sdf_all = q.query_sdf(pts(d_all), sdf_extra(d_all))
            for i, factor in enumerate(upsample_inv_s_factors):
                fine, d_all, order = _row_stage(d_all, sdf_all, q.num_fine[i], q.upsample_inv_s * factor,
                                                upsample_use_estimate_alpha, perturb)
                if i < q.n_stages - 1:
                    sdf_all = torch.cat([sdf_all, q.query_sdf(pts(fine), sdf_extra(fine))], dim=-1).gather(-1, order.long())
            return d_all
        if upsample_mode == 'direct_use':
            d = depths_coarse_1
            sdf = q.query_sdf(pts(d), sdf_extra(d))
        elif upsample_mode == 'direct_more':
            steps = torch.linspace(0, 1, num_nograd, device=device, dtype=torch.float)
            d = torch.lerp(q.near.unsqueeze(-1), q.far.unsqueeze(-1), steps)
            sdf = _chunked(lambda x, **kw: q.query_sdf(x, kw), dict(x=pts(d), **sdf_extra(d)), chunksize_query)
        else:
            raise RuntimeError(f"Invalid upsample_mode={upsample_mode}")
        return _row_stage(d, sdf, num_fine, q.upsample_inv_s, upsample_use_estimate_alpha, perturb)[1]

    with profile("Upsampling"):
        d_all = upsample()
    with profile("Acquire volume buffer"):
        d_mid = 0.5 * (d_all[..., 1:] + d_all[..., :-1])
        alpha = neus_ray_sdf_to_alpha(q.query_sdf(pts(d_all), sdf_extra(d_all)), q.forward_inv_s)
        if not compression:
            vb = dict(type='batched', rays_inds_hit=rays_inds, num_per_hit=d_mid.size(-1), t=d_mid.to(dtype),
                      opacity_alpha=alpha.to(dtype))
            q.finish(vb, None, lambda: pts(d_mid), q.spread(None, d_mid.shape[-1]))
            return vb, {'render.num_per_ray': d_mid.size(-1)}

        # `pack_infos` is over all tested rays
        pack_infos = get_pack_infos_from_batch(alpha.shape[0], alpha.shape[1], device=device)
        nidx_useful, pack_infos_useful, pidx_useful = packed_volume_render_compression(alpha.flatten(), pack_infos)
        if nidx_useful.numel() == 0:
            return empty, {}
        depths_packed = d_mid.flatten()[pidx_useful]
        vb = dict(type='packed', rays_inds_hit=rays_inds[nidx_useful], pack_infos_hit=pack_infos_useful, t=depths_packed.to(dtype),
                  opacity_alpha=alpha.flatten()[pidx_useful].to(dtype))
        ridx = None                                                       # the ray of every kept sample: only the full query asks
        if with_rgb or with_normal:
            ridx = torch.arange(alpha.shape[0], device=device).unsqueeze(-1).expand_as(alpha).flatten()[pidx_useful]
        q.finish(vb, nidx_useful, lambda: torch.addcmul(rays_o[ridx], rays_d[ridx], depths_packed.unsqueeze(-1)), lambda t: t[ridx])
        return vb, {'render.num_per_ray0': d_mid.size(-1), 'render.num_per_ray': pack_infos_useful[:, 1]}


def neus_ray_query_march_occ_multi_upsample(
        model, ray_tested: Dict[str, torch.Tensor],
        with_rgb: bool = True, with_normal: bool = True, perturb: bool = False, nablas_has_grad: bool = False,
        forward_inv_s: float = None,
        num_coarse: int = 0, coarse_step_cfg=dict(step_mode='linear'), chunksize_query: int = 2 ** 24, march_cfg=dict(),
        num_fine: int = 8, upsample_inv_s: float = 64., upsample_s_divisor: float = 1.0,
        upsample_inv_s_factors: List[int] = [1, 4, 16], upsample_use_estimate_alpha=False,
        debug_query_data: dict = None) -> Tuple[dict, dict]:
    _check_model(model)
    empty = dict(type='empty', rays_inds_hit=[])
    if ray_tested['num_rays'] == 0:
        return empty, {}
    q = _setup(model, ray_tested, with_rgb, with_normal, nablas_has_grad, forward_inv_s, num_fine, upsample_inv_s,
               upsample_s_divisor, upsample_inv_s_factors)
    rays_o, rays_d, rays_inds, dtype, forward_inv_s = q.rays_o, q.rays_d, q.rays_inds, q.dtype, q.forward_inv_s
    depths_coarse_1, deltas_coarse_1, marched, depths_1, upsample_stages = _march_and_upsample(
        q, perturb, num_coarse, coarse_step_cfg, chunksize_query, march_cfg, upsample_inv_s_factors, upsample_use_estimate_alpha,
        want_stages=debug_query_data is not None)
    hit = marched.ridx_hit

    with profile("Acquire volume buffer"):
        if hit is None:
            if num_coarse == 0:
                return empty, {}
            # nothing marched: a batched buffer of the coarse samples on every ray
            pts = lambda d: torch.addcmul(rays_o[..., None, :], rays_d[..., None, :], d[..., None])
            sdf = q.query_sdf(pts(depths_coarse_1), q.sdf_attrs(q.spread(None, num_coarse + 1)))
            depths = depths_coarse_1[..., :num_coarse] + deltas_coarse_1[..., :num_coarse] / 2.
            vb = dict(type='batched', rays_inds_hit=rays_inds, num_per_hit=num_coarse, t=depths.to(dtype),
                      opacity_alpha=neus_ray_sdf_to_alpha(sdf, forward_inv_s).to(dtype))
            q.finish(vb, None, lambda: pts(depths), q.spread(None, num_coarse))
            return vb, {'render.num_per_ray': num_coarse}

        details = {'march.num_per_ray': marched.pack_infos[:, 1]}
        if num_coarse == 0:
            # batched buffer: the fine depths are interval boundaries, samples sit at the interval mid-points
            rays_inds_hit = rays_inds[hit]
            o_hit, d_hit = rays_o[hit].unsqueeze(-2), rays_d[hit].unsqueeze(-2)
            sdf = _sdf_maybe_chunked(q, torch.addcmul(o_hit, d_hit, depths_1.unsqueeze(-1)), q.sdf_attrs(q.spread(hit, depths_1.shape[-1])),
                                     chunksize_query)
            depths = depths_1[..., :-1] + depths_1.diff(dim=-1) / 2.
            if debug_query_data is not None:
                debug_query_data["fine"] = dict(ridx=rays_inds_hit[..., None].expand_as(depths).flatten(),
                                                depth=depths_1.data.to(dtype).flatten(), sdf=sdf.data.to(dtype).flatten(),
                                                upsample_stages=upsample_stages.flatten())
            vb = dict(type='batched', rays_inds_hit=rays_inds_hit, num_per_hit=depths.size(-1), t=depths.to(dtype),
                      opacity_alpha=neus_ray_sdf_to_alpha(sdf, forward_inv_s).to(dtype))
            q.finish(vb, hit, lambda: torch.addcmul(o_hit, d_hit, depths[..., None]), q.spread(hit, depths.shape[-1]))
            details['render.num_per_ray'] = depths.size(-1)
            return vb, details

        # packed buffer over ALL tested rays: coarse boundaries of every ray + fine depths of the hit rays
        ridx_all, depths_1p, pack_infos, stages_p = _join_coarse(depths_coarse_1, hit, depths_1, upsample_stages)
        o_p, d_p = rays_o[ridx_all], rays_d[ridx_all]
        sdf_p = q.query_sdf(torch.addcmul(o_p, d_p, depths_1p.unsqueeze(-1)), q.sdf_attrs(lambda t: t[ridx_all]))
        depths_p = depths_1p + packed_diff(depths_1p, pack_infos) / 2.
        if debug_query_data is not None:
            for name, sel in (("coarse", (stages_p == 0).nonzero(as_tuple=True)[0]),
                              ("fine", (stages_p > 0).nonzero(as_tuple=True)[0])):
                debug_query_data[name] = dict(ridx=ridx_all[sel], depth=depths_1p.data.to(dtype)[sel],
                                              sdf=sdf_p.data.to(dtype)[sel])
            debug_query_data["fine"]["upsample_stages"] = stages_p[(stages_p > 0).nonzero(as_tuple=True)[0]]
        vb = dict(type='packed', rays_inds_hit=rays_inds, pack_infos_hit=pack_infos, t=depths_p.to(dtype),
                  opacity_alpha=neus_packed_sdf_to_alpha(sdf_p, forward_inv_s, pack_infos).to(dtype))
        q.finish(vb, None, lambda: torch.addcmul(o_p, d_p, depths_p.unsqueeze(-1)), lambda t: t[ridx_all])
        details['render.num_per_ray'] = pack_infos[:, 1]
        return vb, details


def neus_ray_query_march_occ_multi_upsample_compressed(
        model, ray_tested: Dict[str, torch.Tensor],
        with_rgb: bool = True, with_normal: bool = True, perturb: bool = False, nablas_has_grad: bool = False,
        forward_inv_s: float = None,
        num_coarse: int = 0, coarse_step_cfg=dict(step_mode='linear'), chunksize_query: int = 2 ** 24, march_cfg=dict(),
        num_fine: int = 8, upsample_inv_s: float = 64., upsample_s_divisor: float = 1.0,
        upsample_inv_s_factors: List[int] = [1, 4, 16], upsample_use_estimate_alpha=False) -> Tuple[dict, dict]:
    """The same up-sampling, then ``packed_volume_render_compression`` on the opacities of the final samples: only the
    samples that can still contribute (before early stop, above the alpha threshold) are kept -- always a packed
    buffer over the rays that keep at least one sample -- and only those are sent through the full ``model.forward``
    (nr3d_lib/graphics/neus/neus_ray_query.py:732-1104).  The reference's coarse + fine branch indexes the per-hit-ray
    extras (``rays_pix_hit`` ...) with all-ray indices (:995-997); the per-ray tensors are indexed here."""
    _check_model(model)
    empty = dict(type='empty', rays_inds_hit=[])
    if ray_tested['num_rays'] == 0:
        return empty, {}
    q = _setup(model, ray_tested, with_rgb, with_normal, nablas_has_grad, forward_inv_s, num_fine, upsample_inv_s,
               upsample_s_divisor, upsample_inv_s_factors)
    rays_o, rays_d, rays_inds, device, dtype, forward_inv_s = q.rays_o, q.rays_d, q.rays_inds, q.device, q.dtype, q.forward_inv_s
    depths_coarse_1, deltas_coarse_1, marched, depths_1, _ = _march_and_upsample(
        q, perturb, num_coarse, coarse_step_cfg, chunksize_query, march_cfg, upsample_inv_s_factors, upsample_use_estimate_alpha)
    hit = marched.ridx_hit

    def compressed_buffer(alpha, depths, ridx, pack_infos, rays_of_packs, details):
        """alpha / depths / ridx: flat per sample (ridx = index into the tested rays), packs described by pack_infos;
        rays_of_packs: the tested ray of every pack (None: pack p is ray p)"""
        nidx_useful, pack_infos_useful, pidx_useful = packed_volume_render_compression(alpha, pack_infos)
        if nidx_useful.numel() == 0:
            return empty, {}
        depths, alpha, ridx = depths[pidx_useful], alpha[pidx_useful], ridx[pidx_useful]
        rays_useful = nidx_useful if rays_of_packs is None else rays_of_packs[nidx_useful]
        vb = dict(type='packed', rays_inds_hit=rays_inds[rays_useful], pack_infos_hit=pack_infos_useful,
                  t=depths.to(dtype), opacity_alpha=alpha.to(dtype))
        q.finish(vb, rays_useful, lambda: torch.addcmul(rays_o[ridx], rays_d[ridx], depths.unsqueeze(-1)), lambda t: t[ridx])
        details['render.num_per_ray'] = pack_infos_useful[:, 1]
        return vb, details

    with profile("Acquire volume buffer"):
        if hit is None:
            if num_coarse == 0:
                return empty, {}
            x = torch.addcmul(rays_o[..., None, :], rays_d[..., None, :], depths_coarse_1[..., None])
            sdf = _sdf_maybe_chunked(q, x, q.sdf_attrs(q.spread(None, num_coarse + 1)), chunksize_query)
            alpha = neus_ray_sdf_to_alpha(sdf, forward_inv_s)
            depths = depths_coarse_1[..., :num_coarse] + deltas_coarse_1[..., :num_coarse] / 2.
            n = rays_inds.numel()
            ridx = torch.arange(n, device=device).unsqueeze(-1).expand_as(depths).flatten()
            return compressed_buffer(alpha.flatten(), depths.flatten(), ridx, get_pack_infos_from_batch(n, depths.size(-1), device=device),
                                     None, {'render.num_per_ray0': depths.size(-1)})

        details = {'march.num_per_ray': marched.pack_infos[:, 1]}
        if num_coarse == 0:
            o_hit, d_hit = rays_o[hit].unsqueeze(-2), rays_d[hit].unsqueeze(-2)
            sdf = _sdf_maybe_chunked(q, torch.addcmul(o_hit, d_hit, depths_1.unsqueeze(-1)), q.sdf_attrs(q.spread(hit, depths_1.shape[-1])),
                                     chunksize_query)
            alpha = neus_ray_sdf_to_alpha(sdf, forward_inv_s)
            depths = depths_1[..., :-1] + depths_1.diff(dim=-1) / 2.
            details['render.num_per_ray0'] = depths.size(-1)
            return compressed_buffer(alpha.flatten(), depths.flatten(), hit.unsqueeze(-1).expand_as(depths).flatten(),
                                     get_pack_infos_from_batch(marched.num_hit_rays, depths.size(-1), device=device), hit, details)

        # coarse boundaries of every ray + fine depths of the hit rays, merged per ray; then compressed
        ridx_all, depths_1p, pack_infos, _ = _join_coarse(depths_coarse_1, hit, depths_1)
        depths_p = depths_1p + packed_diff(depths_1p, pack_infos) / 2.
        sdf_p = _sdf_maybe_chunked(q, torch.addcmul(rays_o[ridx_all], rays_d[ridx_all], depths_1p.unsqueeze(-1)),
                                   q.sdf_attrs(lambda t: t[ridx_all]), chunksize_query)
        alpha_p = neus_packed_sdf_to_alpha(sdf_p, forward_inv_s, pack_infos)
        details['render.num_per_ray0'] = pack_infos[:, 1]
        return compressed_buffer(alpha_p, depths_p, ridx_all, pack_infos, None, details)


def neus_ray_query_march_occ_multi_upsample_compressed_strategy(model, ray_tested: Dict[str, torch.Tensor], **kwargs):
    """declared but unimplemented in the reference as well (neus_ray_query.py:1106-1117 raises after resolving inv_s)"""
    _ = model.forward_inv_s() if kwargs.get('forward_inv_s') is None else kwargs['forward_inv_s']
    raise NotImplementedError


def neus_ray_query_sphere_trace(
        model, ray_tested: Dict[str, torch.Tensor], *,
        # Common params
        with_rgb: bool = True, with_normal: bool = True, perturb: bool = False, nablas_has_grad: bool = False,
        # Distinct params
        debug: bool = False, **sphere_trace_cfg) -> Tuple[dict, dict]:
    """Surface rendering by sphere tracing: one hit per ray instead of volume samples (nr3d_lib/graphics/neus/neus_ray_query.py:41-130).
    The model's occupancy grid (``model.accel.occ.resolution`` / ``.occ_grid``) becomes the tracer's ``DenseGrid``, ``model.forward_sdf``
    its distance function; ``sphere_trace_cfg`` goes to ``graphics.sphere_trace.SphereTracer``.  The volume buffer is batched with
    ``num_per_hit=1``: ``t``, ``opacity_alpha`` (1 on the hit rays), ``net_x`` (the hit points), ``nablas`` / ``rgb`` from
    ``model.forward`` at the hit points, ``rays_bidx_hit`` for batched models.
    With zero rays, and with no ray hit, the result is the ``(empty_buffer, {})`` pair -- the reference returns the bare buffer from
    the first of its two early exits, which its callers cannot unpack."""
    _check_model(model)
    use_ts, use_fidx, use_bidx = _flag(model, 'use_ts'), _flag(model, 'use_fidx'), _flag(model, 'use_bidx')
    use_pix = (_flag(model, 'use_pix') and with_rgb) or _flag(model, 'fwd_sdf_use_pix')
    use_h_appear = (_flag(model, 'use_h_appear') and with_rgb) or _flag(model, 'fwd_sdf_use_h_appear')
    use_view_dirs = (_flag(model, 'use_view_dirs') and with_rgb) or _flag(model, 'fwd_sdf_use_view_dirs')

    empty_buffer = dict(type="empty", rays_inds_hit=[])
    if ray_tested["num_rays"] == 0:
        return empty_buffer, {}
    assert ray_tested["rays_o"].dim() == 2

    from nr3d_lib_amd.graphics.sphere_trace import DenseGrid, SphereTracer
    model.tracer = SphereTracer(DenseGrid(*model.accel.occ.resolution, model.accel.occ.occ_grid), **sphere_trace_cfg)
    rays_to_trace = {"rays_o": ray_tested["rays_o"], "rays_d": ray_tested["rays_d"], "near": ray_tested["near"],
                     "far": ray_tested["far"]}
    ret_st = model.tracer.trace(rays_to_trace, model.forward_sdf, print_debug_log=debug)
    hit = ret_st["idx"]
    if hit.numel() == 0:
        return empty_buffer, {}

    with profile("Acquire volume buffer"):
        near, rays_o = ray_tested["near"], ray_tested["rays_o"]
        volume_buffer = dict(type="batched", rays_inds_hit=ray_tested["rays_inds"], num_per_hit=1,
                             t=torch.zeros_like(near)[:, None], opacity_alpha=torch.zeros_like(near)[:, None])
        volume_buffer["opacity_alpha"][hit] = 1.
        if use_bidx:
            volume_buffer['rays_bidx_hit'] = torch.full_like(near, -1)[:, None]
            volume_buffer['rays_bidx_hit'][hit] = ray_tested['rays_bidx'][hit]
        if with_rgb or with_normal:
            fwd_kwargs = dict(x=ret_st["pos"], nablas_has_grad=nablas_has_grad, with_rgb=with_rgb, with_normal=with_normal)
            # Extra infos attached to each ray
            for on, (arg, key) in zip((use_ts, use_fidx, use_bidx, use_pix, use_h_appear), _RAY_ATTRS):
                if on:
                    fwd_kwargs[arg] = ray_tested[key][hit]
            if use_view_dirs:
                fwd_kwargs['v'] = F.normalize(ret_st["dir"], 2, -1)
            net_out = model.forward(**fwd_kwargs)
            volume_buffer["net_x"] = torch.zeros_like(rays_o)[:, None]
            volume_buffer["net_x"][hit] = ret_st["pos"][:, None]
            if "nablas" in net_out:
                volume_buffer["nablas"] = torch.zeros_like(rays_o)[:, None]
                volume_buffer["nablas"][hit] = net_out["nablas"][:, None].to(volume_buffer["nablas"].dtype)
            if "rgb" in net_out:
                volume_buffer["rgb"] = rays_o.new_zeros(rays_o.shape[0], 1, net_out["rgb"].shape[-1])
                volume_buffer["rgb"][hit] = net_out["rgb"][:, None].to(volume_buffer["rgb"].dtype)
        details = {'render.num_per_ray': 1}
    return volume_buffer, details
