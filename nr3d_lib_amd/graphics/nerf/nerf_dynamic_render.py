"""Decomposed render of a static + dynamic field (EmerNeRF's ``with_static_dynamic`` / ``with_flow``): the volume buffer of a ray query
whose network returns ``sigma_static`` / ``sigma_dynamic`` (and ``rgb_*``, ``nablas_*``, the flows) next to the combined outputs ->
the per-ray ``mask_/depth_/rgb_/normals_{static,dynamic}`` and the flows rendered with the DYNAMIC weights.  Model-independent code
that lives inside a model class in the reference (nr3d_lib/models/fields_dynamic/nerf/emernerf.py:806-938).

Packed buffers run on the library's fused entries: ``sigma_delta_to_alpha`` (tau_to_alpha), ``packed_composite`` /
``packed_composite_normals`` once per side, ``packed_sum`` for the flows.  'batched' buffers never arise from the march-based queries
and stay torch ops."""
import torch

from nr3d_lib_amd import _hip as _H
from nr3d_lib_amd.graphics.nerf.nerf_utils import sigma_delta_to_alpha
from nr3d_lib_amd.graphics.neus.neus_render import _packed_sum_torch, _ray_chain, _scatter, packed_composite_normals
from nr3d_lib_amd.graphics.pack_ops import packed_sum

__all__ = ['composite_static_dynamic', 'FLOW_KEYS']

FLOW_KEYS = ('flow_fwd', 'flow_fwd_pred_bwd', 'flow_bwd', 'flow_bwd_pred_fwd')


def _side_alphas(volume_buffer):
    """opacity_alpha_static / _dynamic, from the side's density where the query did not provide them (emernerf.py:806-811)"""
    for side in ('static', 'dynamic'):
        if 'opacity_alpha_' + side not in volume_buffer:
            volume_buffer['opacity_alpha_' + side] = sigma_delta_to_alpha(volume_buffer['sigma_' + side], volume_buffer['deltas'])


def composite_static_dynamic(volume_buffer: dict, num_rays: int, with_rgb: bool = True, with_normal: bool = False,
                             with_flow: bool = False, training: bool = True, depth_use_normalized_vw: bool = True, device=None,
                             dtype=torch.float32) -> dict:
    """-> {'mask_static', 'mask_dynamic', 'depth_static', 'depth_dynamic' [num_rays]; 'rgb_static', 'rgb_dynamic' [num_rays, 3]
    (``with_rgb``); 'normals_static', 'normals_dynamic' [num_rays, 3] (``with_normal``; zeros where the buffer has no ``nablas_<side>``);
    'flow_fwd', 'flow_bwd' and whichever of the ``*_pred_*`` flows the buffer holds [num_rays, 3] (``with_flow``)}.  Rays the buffer does
    not hit are zero.  Sets ``volume_buffer['opacity_alpha_<side>']`` (when absent) and ``volume_buffer['vw_<side>']``.  ``training``
    False: normals are clamped (in place) and normalised, as in ``composite_volume_buffer``."""
    num_rays = int(num_rays)
    buffer_type = volume_buffer['type']
    if buffer_type not in ('empty', 'batched', 'packed'):
        raise RuntimeError(f"composite_static_dynamic: unknown volume buffer type {buffer_type!r}")
    if device is None:
        device = next((v.device for v in volume_buffer.values() if isinstance(v, torch.Tensor)), None)
    zeros = lambda *tail: torch.zeros(num_rays, *tail, dtype=dtype, device=device)      # noqa: E731
    out = {}
    for side in ('static', 'dynamic'):
        out['mask_' + side], out['depth_' + side] = zeros(), zeros()
        if with_rgb:
            out['rgb_' + side] = zeros(3)
        if with_normal:
            out['normals_' + side] = zeros(3)
    if with_flow:
        out['flow_fwd'], out['flow_bwd'] = zeros(3), zeros(3)
    if buffer_type == 'empty':
        return out

    _side_alphas(volume_buffer)
    t, hit = volume_buffer['t'], volume_buffer['rays_inds_hit']
    packed = buffer_type == 'packed'
    if packed:
        pack_infos = volume_buffer['pack_infos_hit']
        tiles = _H.tiles(pack_infos, t.numel())
    for side in ('static', 'dynamic'):
        alpha = volume_buffer['opacity_alpha_' + side]
        rgb = volume_buffer['rgb_' + side] if with_rgb else None
        nablas = volume_buffer.get('nablas_' + side) if with_normal else None
        if packed:
            vw, mask, depth, rgb_out, normals = packed_composite_normals(
                alpha, t, rgb, nablas, pack_infos, hit, num_rays, normalize_depth=depth_use_normalized_vw, packs_tile=tiles,
                normalized_normals=not training)
        else:
            vw, mask, depth, rgb_out, normals = _ray_chain(alpha, t, rgb, nablas, hit, num_rays, depth_use_normalized_vw, not training)
        volume_buffer['vw_' + side] = vw
        out['mask_' + side], out['depth_' + side] = mask, depth
        if with_rgb:
            out['rgb_' + side] = rgb_out
        if normals is not None:
            out['normals_' + side] = normals
    if with_flow:
        vw = volume_buffer['vw_dynamic']        # flows are only valid for the dynamic part
        for k in FLOW_KEYS:
            if k not in volume_buffer:
                continue
            flow = volume_buffer[k]
            if not packed:
                out[k] = _scatter((vw.unsqueeze(-1) * flow).sum(dim=-2), hit, num_rays)
                continue
            weighted = vw.view(-1, 1) * flow.view(-1, 3)
            lib = weighted.is_cuda and (tiles or not (torch.is_grad_enabled() and weighted.requires_grad))
            out[k] = _scatter((packed_sum if lib else _packed_sum_torch)(weighted, pack_infos), hit, num_rays)
    return out
