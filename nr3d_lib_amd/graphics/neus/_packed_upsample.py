"""The multi-factor up-sampling of the NeuS occupancy-march queries on packed samples, stated once for both model kinds: the
single-block drivers of ``neus_ray_query`` (no labels) and the forest drivers of ``neus_forest_ray_query`` (every sample carries
the index of its block).  Per factor: CDF positions, one launch of the packed stage (``bindings._neus_upsample``) or the reference's
pack-op chain, the SDF at the new depths, their sorted union with the packed buffer, the next, sharper factor.

What stays with the callers: the first (chunked) SDF query, the final sort of the new depths, and the union behind the last
factor, which nothing but the forest's coarse driver reads (``union``)."""
import torch

from nr3d_lib_amd.bindings import _neus_upsample
from nr3d_lib_amd.graphics.nerf.nerf_utils import packed_alpha_to_vw
from nr3d_lib_amd.graphics.neus.neus_utils import neus_packed_sdf_to_alpha, neus_packed_sdf_to_upsample_alpha
from nr3d_lib_amd.graphics.pack_ops import (get_pack_infos_from_batch, merge_two_packs_sorted_aligned, packed_cumsum, packed_div,
                                            packed_invert_cdf)
from nr3d_lib_amd.graphics.raysample import cdf_positions


def union(depth, blidx, pack_infos, fine, blidx_fine):
    """the new depths [P, m] and their labels joined to the packed ones, sorted per pack (a new depth before an equal old one);
    blidx, blidx_fine None: no labels -> (depth, blidx | None, pack_infos, pidx of the old, pidx of the new elements)"""
    pinfo_fine = get_pack_infos_from_batch(fine.shape[0], fine.shape[1], device=fine.device)
    pidx0, pidx1, pinfo = merge_two_packs_sorted_aligned(depth, pack_infos, fine.flatten(), pinfo_fine, b_sorted=True, return_val=False)
    total = depth.numel() + fine.numel()
    d_new = depth.new_empty([total])
    d_new[pidx0], d_new[pidx1] = depth, fine.flatten()
    b_new = None
    if blidx is not None:
        b_new = blidx.new_empty([total])
        b_new[pidx0], b_new[pidx1] = blidx, blidx_fine.flatten()
    return d_new, b_new, pinfo, pidx0, pidx1


@torch.no_grad()
def upsample_loop(o_packs, d_packs, depth, sdf, pack_infos, blidx, num_fine, factors, upsample_inv_s, use_estimate_alpha, perturb,
                  fused, sdf_at):
    """o_packs, d_packs [P, 3]: the ray of every pack; depth, sdf [N] packed by pack_infos [P, 2], which tile [0, N); blidx int64 [N]
    or None: a label per sample.  Factor i draws ``num_fine[i]`` new depths per pack from the up-sampling CDF at
    ``upsample_inv_s * factors[i]``, each with the label of the upper end of its CDF bin; behind every factor but the last they join
    the packed buffer, and ``sdf_at(x [P, m, 3], labels [P, m] | None)`` gives their SDF (P m values, cast to the buffer's dtype).
    ``fused``: one launch of the packed stage per factor for float32 samples on the GPU (int64 labels), no union on the last factor;
    otherwise, and for every other input, the reference's pack-op chain.  Both invert at the same ``cdf_positions``, drawn once per
    factor before that factor's SDF query.
    -> (the new depths per factor [P, num_fine[i]], their labels likewise | None, (depth, blidx, pack_infos) as the last factor saw
    them)"""
    n_stages, P, labelled = len(factors), pack_infos.shape[0], blidx is not None
    o_packs, d_packs = o_packs.unsqueeze(-2), d_packs.unsqueeze(-2)
    fines, blidx_fines = [], []
    fused = fused and depth.is_cuda and depth.dtype == torch.float32 and sdf.dtype == torch.float32 \
        and (not labelled or blidx.dtype == torch.int64)
    for i, factor in enumerate(factors):
        inv_s, m, more = upsample_inv_s * factor, num_fine[i], i < n_stages - 1
        u = cdf_positions(depth, (P,), m, perturb)
        blidx_fine = blidx_m = None
        if fused and not labelled:
            fine, merged, sdf_m, pidx1, pinfo = _neus_upsample.upsample_stage_packed(
                depth.contiguous(), sdf.contiguous(), pack_infos, u, inv_s, use_estimate_alpha, merge=more, need_sdf=more)
        elif fused:
            fine, blidx_fine, merged, sdf_m, blidx_m, pidx1, pinfo = _neus_upsample.upsample_stage_packed_blocks(
                depth.contiguous(), sdf.contiguous(), blidx.contiguous(), pack_infos, u, inv_s, use_estimate_alpha, merge=more,
                need_sdf=more)
        else:
            # the reference's op chain (fused=False: no kernel of neus_utils.FUSED_SDF_TO_ALPHA either)
            alpha = (neus_packed_sdf_to_upsample_alpha(sdf, depth, inv_s, pack_infos) if use_estimate_alpha
                     else neus_packed_sdf_to_alpha(sdf, inv_s, pack_infos, fused=False))
            cdf = packed_cumsum(packed_alpha_to_vw(alpha, pack_infos), pack_infos, exclusive=True)
            last = cdf[pack_infos[..., 0] + pack_infos[..., 1] - 1]
            cdf = packed_div(cdf, last.clamp_min(1e-5), pack_infos)
            fine, pidx_bin = packed_invert_cdf(depth, cdf.to(depth.dtype), u.expand(P, m).contiguous(), pack_infos)
            if labelled:
                blidx_fine = blidx[pidx_bin]
        fines.append(fine)
        blidx_fines.append(blidx_fine)
        if not more:
            break
        sdf_fine = sdf_at(torch.addcmul(o_packs, d_packs, fine.unsqueeze(-1)), blidx_fine).flatten()
        if fused:
            sdf_m[pidx1.flatten()] = sdf_fine.to(sdf_m.dtype)
        else:
            merged, blidx_m, pinfo, pidx0, pidx1 = union(depth, blidx, pack_infos, fine, blidx_fine)
            sdf_m = sdf.new_empty([merged.numel()])
            sdf_m[pidx0], sdf_m[pidx1] = sdf, sdf_fine.to(sdf.dtype)
        depth, sdf, blidx, pack_infos = merged, sdf_m, blidx_m, pinfo
    return fines, (blidx_fines if labelled else None), (depth, blidx, pack_infos)
