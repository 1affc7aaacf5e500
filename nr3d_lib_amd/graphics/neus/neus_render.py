"""The last stage of a NeuS render: the volume buffer of a ray query -> ``vw``, ``mask_volume``, ``depth_volume``, ``rgb_volume`` and
``normals_volume`` -- the block at the end of ``NeusRendererMixin.ray_query`` (nr3d_lib/models/fields/neus/renderer_mixin.py:396-439)
as a function, for the 'batched' buffers of the coarse / sphere-trace queries and the 'packed' ones of the march-occ queries.

Two routes with the same semantics: one launch of the HIP kernels each way (``bindings._neus_composite``, ``NeusComposite``), or the
reference's chain of torch ops, written out below (``_ray_chain`` / ``_packed_chain``) as the cross-check and for every input the
kernels do not take.  Rows follow ``ray_alpha_to_vw`` (no early stop); packs follow ``packed_alpha_to_vw`` with its defaults
(``early_stop_eps`` 1e-4, ``alpha_thre`` 0), as ``packed_composite`` does.

Normals: ``training`` composites the raw ``nablas``; evaluation clamps them to [-1, 1] IN PLACE (the reference's ``clamp_``: the buffer
the caller holds afterwards is the clamped one) and composites the unit vectors.  The kernels have no backward for the second form, so
it takes the fused route only where no gradient is recorded."""
import torch
import torch.nn.functional as F

from nr3d_lib_amd import _hip as _H
from nr3d_lib_amd.bindings import _neus_composite as _backend
from nr3d_lib_amd.graphics.nerf.nerf_utils import ray_alpha_to_vw
from nr3d_lib_amd.graphics.pack_ops import packed_alpha_to_vw, packed_composite, packed_div, packed_sum

__all__ = ['NeusComposite', 'ray_composite', 'packed_composite_normals', 'composite_volume_buffer']


# ray_composite / packed_composite_normals / composite_volume_buffer: True = one launch of the HIP kernels each way for float32 GPU
# tensors; False (and every other input: CPU tensors, other dtypes, normalised normals while a gradient is recorded) = the
# reference's torch op chain.  Same semantics.  The default follows profiles/neus_composite.json (tools/exp_neus_composite.py).
FUSED_NEUS_COMPOSITE = True


class NeusComposite(torch.autograd.Function):
    """vw, mask, depth, rgb and normals of a volume buffer as one kernel each way.  ``layout`` = (pack_infos | None, rays_inds_hit | None,
    num_rays, early_stop_eps, alpha_thre, normalize_depth, normals_mode, packs_tile): not tensors for autograd.
    -> (vw, mask, depth, rgb_out | None, normals_out | None); all are differentiable with respect to alpha, t, rgb and nablas."""

    @staticmethod
    def forward(ctx, alpha, t, rgb, nablas, layout):
        pack_infos, rays_inds_hit, num_rays, eps, thre, normalize, mode, packs_tile = layout
        vw, mask, depth, rgb_out, normals_out = _backend.neus_composite_forward(alpha, t, rgb, nablas, pack_infos, rays_inds_hit, num_rays,
                                                                                eps, thre, normalize, mode, packs_tile)
        ctx.save_for_backward(alpha, t, rgb, nablas, vw, mask, depth)
        ctx.layout = layout
        ctx.set_materialize_grads(False)
        return vw, mask, depth, rgb_out, normals_out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_vw, g_mask, g_depth, g_rgb, g_normals):
        alpha, t, rgb, nablas, vw, mask, depth = ctx.saved_tensors
        pack_infos, rays_inds_hit, _, eps, thre, normalize, mode, packs_tile = ctx.layout
        need = ctx.needs_input_grad
        c = lambda g: None if g is None else g.contiguous()     # noqa: E731
        ga, gt, gr, gn = _backend.neus_composite_backward(alpha, t, rgb, nablas, pack_infos, rays_inds_hit, eps, thre, normalize, mode,
                                                          vw, mask, depth, c(g_mask), c(g_depth), c(g_rgb), c(g_normals), c(g_vw),
                                                          need_t=need[1], need_rgb=need[2], need_nablas=need[3], packs_tile=packs_tile)
        return ga if need[0] else None, gt, gr, gn, None


def _fused(alpha, t, rgb, nablas, normalized_normals):
    """whether the kernels take this call: the switch, float32 GPU tensors, and no gradient wanted through the normalised normals"""
    if not FUSED_NEUS_COMPOSITE:
        return False
    tensors = [x for x in (alpha, t, rgb, nablas) if x is not None]
    if not all(x.is_cuda and x.dtype == torch.float32 for x in tensors):
        return False
    if normalized_normals and nablas is not None and torch.is_grad_enabled() and any(x.requires_grad for x in tensors):
        return False
    return True


def _apply(alpha, t, rgb, nablas, layout):
    c = lambda x: None if x is None else x.contiguous()     # noqa: E731
    alpha, t, rgb, nablas = c(alpha), c(t), c(rgb), c(nablas)
    if torch.is_grad_enabled() and any(x is not None and x.requires_grad for x in (alpha, t, rgb, nablas)):
        return NeusComposite.apply(alpha, t, rgb, nablas, layout)
    d = lambda x: None if x is None else x.detach()         # noqa: E731
    pack_infos, rays_inds_hit, num_rays, eps, thre, normalize, mode, packs_tile = layout
    return _backend.neus_composite_forward(d(alpha), d(t), d(rgb), d(nablas), pack_infos, rays_inds_hit, num_rays, eps, thre, normalize,
                                           mode, packs_tile)


def _unit_normals(nablas):
    """evaluation normals: clamped IN PLACE as the reference does, then unit length"""
    return F.normalize(nablas.clamp_(-1, 1), dim=-1)


def _scatter(x, rays_inds_hit, num_rays):
    if rays_inds_hit is None:
        return x
    out = x.new_zeros((num_rays, *x.shape[1:]))
    out[rays_inds_hit] = x
    return out


def _ray_chain(alpha, t, rgb, nablas, rays_inds_hit, num_rays, normalize_depth, normalized_normals):
    """renderer_mixin.py:403-419"""
    vw = ray_alpha_to_vw(alpha)
    vw_sum = vw.sum(dim=-1)
    if normalize_depth:
        depth = ((vw / (vw_sum.unsqueeze(-1) + 1e-10)) * t).sum(dim=-1)
    else:
        depth = (vw * t).sum(dim=-1)
    rgb_out = None if rgb is None else (vw.unsqueeze(-1) * rgb).sum(dim=-2)
    normals = None
    if nablas is not None:
        normals = (vw.unsqueeze(-1) * (_unit_normals(nablas) if normalized_normals else nablas)).sum(dim=-2)
    s = lambda x: None if x is None else _scatter(x, rays_inds_hit, num_rays)      # noqa: E731
    return vw, s(vw_sum), s(depth), s(rgb_out), s(normals)


def _pack_rows(pack_infos):
    """(sample index of every sample inside a pack, its pack's index), pack by pack"""
    first, lens = pack_infos[:, 0], pack_infos[:, 1]
    pid = torch.repeat_interleave(torch.arange(pack_infos.shape[0], device=pack_infos.device), lens)
    within = torch.arange(pid.shape[0], device=pack_infos.device) - (lens.cumsum(0) - lens)[pid]
    return first[pid] + within, pid


def _packed_alpha_to_vw_torch(alpha, pack_infos, early_stop_eps, alpha_thre):
    """packed_alpha_to_vw in torch ops, pack by pack (CPU tensors: the library's pack ops run on the GPU only): a sample with
    alpha <= alpha_thre neither counts nor attenuates, and from the first sample whose transmittance is below early_stop_eps on the
    weights are zero (the transmittance does not rise, so that is a mask); zero outside every pack"""
    pieces = []
    for first, n in pack_infos.tolist():
        if n:
            a = alpha[first:first + n]
            a = torch.where(a > alpha_thre, a, torch.zeros_like(a))
            T = torch.cumprod(torch.cat([a.new_ones(1), 1 - a[:-1]]), dim=0)
            pieces.append(torch.where(T < early_stop_eps, torch.zeros_like(a), a * T))
    if not pieces:
        return torch.zeros_like(alpha)
    return torch.zeros_like(alpha).index_put((_pack_rows(pack_infos)[0],), torch.cat(pieces))


def _packed_sum_torch(x, pack_infos):
    idx, pid = _pack_rows(pack_infos)
    return x.new_zeros((pack_infos.shape[0], *x.shape[1:])).index_add(0, pid, x[idx])


def _packed_div_torch(x, per_pack, pack_infos):
    """x / its pack's value; samples outside every pack are zero, as packed_div's"""
    idx, pid = _pack_rows(pack_infos)
    return torch.zeros_like(x).index_put((idx,), x[idx] / per_pack[pid])


def _packed_chain(alpha, t, rgb, nablas, pack_infos, rays_inds_hit, num_rays, early_stop_eps, alpha_thre, normalize_depth,
                  normalized_normals):
    """renderer_mixin.py:421-439.  On the GPU with the library's pack ops; the backward of its packed_sum / packed_div takes packs that
    tile the buffer only, so where a gradient is recorded and the packs are not known to tile (``_hip.tiles``) the sums and the division
    are the index-op restatements below, which take gaps; CPU tensors always do."""
    if alpha.is_cuda:
        vw = packed_alpha_to_vw(alpha, pack_infos, early_stop_eps, alpha_thre)
        grad = torch.is_grad_enabled() and any(x is not None and x.requires_grad for x in (alpha, t, rgb, nablas))
        lib = _H.tiles(pack_infos, alpha.numel()) or not grad
        psum, pdiv = (packed_sum, packed_div) if lib else (_packed_sum_torch, _packed_div_torch)
    else:
        vw = _packed_alpha_to_vw_torch(alpha, pack_infos, early_stop_eps, alpha_thre)
        psum, pdiv = _packed_sum_torch, _packed_div_torch
    vw_sum = psum(vw.view(-1), pack_infos)
    if normalize_depth:
        depth = psum(pdiv(vw, vw_sum + 1e-10, pack_infos) * t.view(-1), pack_infos)
    else:
        depth = psum(vw.view(-1) * t.view(-1), pack_infos)
    rgb_out = None if rgb is None else psum(vw.view(-1, 1) * rgb.view(-1, 3), pack_infos)
    normals = None
    if nablas is not None:
        normals = psum(vw.view(-1, 1) * (_unit_normals(nablas) if normalized_normals else nablas).reshape(-1, 3), pack_infos)
    s = lambda x: None if x is None else _scatter(x, rays_inds_hit, num_rays)      # noqa: E731
    return vw, s(vw_sum), s(depth), s(rgb_out), s(normals)


def ray_composite(alpha, t, rgb=None, nablas=None, rays_inds_hit=None, num_rays=None, normalize_depth=True, normalized_normals=False):
    """alpha composite of a 'batched' volume buffer: alpha, t [R, n]; rgb, nablas [R, n, 3] | None; ``rays_inds_hit`` int64 [R] scatters
    the per-ray results into [num_rays] outputs (other rays stay zero).  -> (vw [R, n], mask, depth, rgb | None, normals | None).
    ``normalized_normals``: the evaluation form, ``nablas`` clamped to [-1, 1] in place."""
    if num_rays is None:
        num_rays = alpha.shape[0]
    if alpha.dim() == 2 and _fused(alpha, t, rgb, nablas, normalized_normals):
        layout = (None, None if rays_inds_hit is None else rays_inds_hit.contiguous(), int(num_rays), 0.0, 0.0, bool(normalize_depth),
                  1 if normalized_normals else 0, False)
        return _apply(alpha, t, rgb, _inplace_target(nablas, normalized_normals), layout)
    return _ray_chain(alpha, t, rgb, nablas, rays_inds_hit, int(num_rays), normalize_depth, normalized_normals)


def packed_composite_normals(alpha, t, rgb, nablas, pack_infos, rays_inds_hit=None, num_rays=None, early_stop_eps: float = 1e-4,
                             alpha_thre: float = 0.0, normalize_depth: bool = True, packs_tile: bool = False,
                             normalized_normals: bool = False):
    """``packed_composite`` with the samples' ``nablas`` [S, 3] composited next to rgb -> (vw, mask, depth, rgb | None, normals | None);
    the arguments and their meaning as there.  ``normalized_normals``: the evaluation form, ``nablas`` clamped to [-1, 1] in place.
    Packs may leave gaps in either route (the op chain falls back to index ops for its sums where the library's have no backward)."""
    if num_rays is None:
        num_rays = pack_infos.shape[0]
    alpha, t = alpha.reshape(-1), t.reshape(-1)
    rgb = None if rgb is None else rgb.reshape(-1, 3)
    if _fused(alpha, t, rgb, nablas, normalized_normals):
        if nablas is None:
            return (*packed_composite(alpha, t, rgb, pack_infos, rays_inds_hit, num_rays, early_stop_eps, alpha_thre, normalize_depth,
                                      packs_tile), None)
        layout = (pack_infos.contiguous(), None if rays_inds_hit is None else rays_inds_hit.contiguous(), int(num_rays),
                  float(early_stop_eps), float(alpha_thre), bool(normalize_depth), 1 if normalized_normals else 0, bool(packs_tile))
        return _apply(alpha, t, rgb, _inplace_target(nablas, normalized_normals, whole=not packs_tile).reshape(-1, 3), layout)
    return _packed_chain(alpha, t, rgb, nablas, pack_infos, rays_inds_hit, int(num_rays), early_stop_eps, alpha_thre, normalize_depth,
                         normalized_normals)


def _inplace_target(nablas, normalized_normals, whole=False):
    """the kernel clamps the samples of the rows or packs of the tensor it is given.  The reference's clamp_ covers the caller's whole
    buffer: a non-contiguous ``nablas`` (the kernel would get a copy) and a packed one whose packs may leave samples out (``whole``) are
    clamped here first, and the kernel's clamp then changes nothing"""
    if nablas is not None and normalized_normals and (whole or not nablas.is_contiguous()):
        nablas.clamp_(-1, 1)
    return nablas


def composite_volume_buffer(volume_buffer, num_rays, with_rgb=True, with_normal=True, training=True, depth_use_normalized_vw=True,
                            device=None, dtype=torch.float32) -> dict:
    """renderer_mixin.py:396-439: -> {'mask_volume' [num_rays], 'depth_volume' [num_rays], 'rgb_volume' [num_rays, 3] (``with_rgb``),
    'normals_volume' [num_rays, 3] (``with_normal``)}; rays the buffer does not hit are zero.  Sets ``volume_buffer['vw']`` for 'batched'
    and 'packed' buffers.  ``training`` False: the normals are clamped and normalised, and ``volume_buffer['nablas']`` is clamped in place."""
    buffer_type = volume_buffer['type']
    num_rays = int(num_rays)
    if buffer_type not in ('empty', 'batched', 'packed'):
        raise RuntimeError(f"composite_volume_buffer: unknown volume buffer type {buffer_type!r}")
    if buffer_type == 'empty':
        if device is None:
            device = next((v.device for v in volume_buffer.values() if isinstance(v, torch.Tensor)), None)
        out = dict(mask_volume=torch.zeros(num_rays, dtype=dtype, device=device), depth_volume=torch.zeros(num_rays, dtype=dtype, device=device))
        if with_rgb:
            out['rgb_volume'] = torch.zeros(num_rays, 3, dtype=dtype, device=device)
        if with_normal:
            out['normals_volume'] = torch.zeros(num_rays, 3, dtype=dtype, device=device)
        return out
    rgb = volume_buffer['rgb'] if with_rgb else None
    nablas = volume_buffer['nablas'] if with_normal else None
    alpha, t, rays_inds_hit = volume_buffer['opacity_alpha'], volume_buffer['t'], volume_buffer['rays_inds_hit']
    if buffer_type == 'batched':
        vw, mask, depth, rgb_out, normals = ray_composite(alpha, t, rgb, nablas, rays_inds_hit, num_rays, depth_use_normalized_vw,
                                                          normalized_normals=not training)
    else:
        pack_infos = volume_buffer['pack_infos_hit']
        vw, mask, depth, rgb_out, normals = packed_composite_normals(alpha, t, rgb, nablas, pack_infos, rays_inds_hit, num_rays,
                                                                     normalize_depth=depth_use_normalized_vw,
                                                                     packs_tile=_H.tiles(pack_infos, alpha.numel()),
                                                                     normalized_normals=not training)
    volume_buffer['vw'] = vw
    out = dict(mask_volume=mask, depth_volume=depth)
    if with_rgb:
        out['rgb_volume'] = rgb_out
    if with_normal:
        out['normals_volume'] = normals
    return out
