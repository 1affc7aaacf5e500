"""nr3d_lib_amd.bindings._neus_upsample -- one up-sampling stage of the NeuS ray queries in one launch (csrc/neus_upsample.hip
through include/nr3d_hip.h): ``upsample_stage`` on the fixed-length rows of the vanilla coarse query, ``upsample_stage_packed`` on
the packs of the occupancy-march queries, ``upsample_stage_packed_blocks`` on packs whose samples carry a block index each (the
forest drivers of ``graphics.neus.neus_forest_ray_query``); the two packed forms are one body over one entry point.

Like ``_mlp`` this module has NO reference twin: the reference runs a stage as a chain of torch ops between two SDF queries
(nr3d_lib/graphics/neus/neus_ray_query.py:258-270).  ``graphics.neus.neus_ray_query.neus_ray_query_coarse_multi_upsample`` is its
caller of the row form, ``graphics.neus._packed_upsample.upsample_loop`` (the march-occ drivers, single-block and forest) of the packed ones.
A CPU tensor raises RuntimeError; there is no fallback here."""
import torch

from .. import _hip as H
from ._args import chk, same_device, u_rows

__all__ = ["MAX_ROW", "PACKED_LDS_ROW", "upsample_stage", "upsample_stage_packed", "upsample_stage_packed_blocks"]


def __getattr__(name):
    """``MAX_ROW``: the library's cap on n + m (NR3D_NEUS_UPSAMPLE_MAX_ROW), asked of the library so that it is stated once"""
    if name == "MAX_ROW":
        return int(H.lib().nr3d_neus_upsample_max_row())
    if name == "PACKED_LDS_ROW":        # packs with len + m up to this are staged in LDS by upsample_stage_packed, longer ones are not
        return int(H.lib().nr3d_neus_upsample_packed_lds_row())
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def upsample_stage(depth, sdf, u, inv_s, use_estimate):
    """depth, sdf float32 [R, n] (depth non-decreasing per row, n >= 2); u float32 [m] (one row of CDF positions for every ray) or
    [R, m] (per ray), non-decreasing, m >= 1; n + m <= MAX_ROW.
    -> (fine [R, m]: the inverse of the row's up-sampling CDF at u, non-decreasing; merged [R, n + m]: the sorted union of depth and
    fine; order int32 [R, n + m]: merged == cat([depth, fine], -1).gather(-1, order), depth elements first on equal values).
    ``use_estimate``: the NeuS paper's slope estimate (neus_ray_sdf_to_upsample_alpha) instead of neus_ray_sdf_to_alpha."""
    fn = "upsample_stage"
    chk(fn, "depth", depth)
    if depth.dim() != 2 or depth.shape[1] < 2:
        raise RuntimeError(f"{fn}: `depth` must be [R, n] with n >= 2, got {list(depth.shape)}")
    R, n = depth.shape
    chk(fn, "sdf", sdf, (R, n))
    m, u_stride = u_rows(fn, u, R)
    dev = depth.device
    same_device(fn, dev, "depth", sdf=sdf, u=u)
    max_row = __getattr__("MAX_ROW")
    if n + m > max_row:
        raise RuntimeError(f"{fn}: n + m = {n + m}, rows of at most MAX_ROW = {max_row} are served")
    if R >= 2 ** 31:
        raise RuntimeError(f"{fn}: {R} rays in one call, the limit is 2^31 - 1 (split the batch)")
    fine = H.empty((R, m), dtype=torch.float32, device=dev)
    merged = H.empty((R, n + m), dtype=torch.float32, device=dev)
    order = H.empty((R, n + m), dtype=torch.int32, device=dev)
    if R:
        with H.on_device(dev):
            H.check(H.lib().nr3d_neus_upsample_stage(R, n, m, H.ptr(depth), H.ptr(sdf), H.ptr(u), u_stride, float(inv_s),
                                                     1 if use_estimate else 0, H.ptr(fine), H.ptr(merged), H.ptr(order),
                                                     H.stream_of(depth)))
    return fine, merged, order


def _stage_packed(fn, labels, depth, sdf, blidx, pack_infos, u, inv_s, use_estimate, merge, need_sdf):
    """the checks, the allocations and the call of both packed forms; without ``labels`` blidx is None, and so are the two label outputs
    -> (fine, blidx_fine, merged, sdf_merged, blidx_merged, pidx_fine, pack_infos_out)"""
    chk(fn, "depth", depth)
    if depth.dim() != 1:
        raise RuntimeError(f"{fn}: `depth` must be [N], got {list(depth.shape)}")
    N = depth.shape[0]
    chk(fn, "sdf", sdf, (N,))
    if labels:
        chk(fn, "blidx", blidx, (N,), torch.int64)
    chk(fn, "pack_infos", pack_infos, None, torch.int64)
    if pack_infos.dim() != 2 or pack_infos.shape[1] != 2:
        raise RuntimeError(f"{fn}: `pack_infos` must be [P, 2], got {list(pack_infos.shape)}")
    P = pack_infos.shape[0]
    m, u_stride = u_rows(fn, u, P)
    dev = depth.device
    same_device(fn, dev, "depth", sdf=sdf, blidx=blidx, pack_infos=pack_infos, u=u)
    if N + P * m >= 2 ** 31:
        raise RuntimeError(f"{fn}: N + P m = {N + P * m}, the merged buffer holds at most 2^31 - 1 elements (split the batch)")
    need_sdf = bool(merge and need_sdf)
    fine = H.empty((P, m), dtype=torch.float32, device=dev)
    blidx_fine = H.empty((P, m), dtype=torch.int64, device=dev) if labels else None
    merged = H.empty((N + P * m,), dtype=torch.float32, device=dev) if merge else None
    sdf_merged = H.empty((N + P * m,), dtype=torch.float32, device=dev) if need_sdf else None
    blidx_merged = H.empty((N + P * m,), dtype=torch.int64, device=dev) if merge and labels else None
    pidx_fine = H.empty((P, m), dtype=torch.int64, device=dev) if merge else None
    pack_infos_out = H.empty((P, 2), dtype=torch.int64, device=dev) if merge else None
    if P:
        workspace = H.empty((max(N, 1),), dtype=torch.float32, device=dev)       # the CDF of the packs that do not fit the LDS row
        with H.on_device(dev):
            H.check(H.lib().nr3d_neus_upsample_stage_packed(
                P, N, m, H.ptr(depth), H.ptr(sdf), H.ptr(blidx), H.ptr(pack_infos), H.ptr(u), u_stride, float(inv_s),
                1 if use_estimate else 0, 1 if merge else 0, 1 if need_sdf else 0, H.ptr(workspace), H.ptr(fine), H.ptr(blidx_fine),
                H.ptr(merged), H.ptr(sdf_merged), H.ptr(blidx_merged), H.ptr(pidx_fine), H.ptr(pack_infos_out), H.stream_of(depth)))
    return fine, blidx_fine, merged, sdf_merged, blidx_merged, pidx_fine, pack_infos_out


def upsample_stage_packed(depth, sdf, pack_infos, u, inv_s, use_estimate, merge=True, need_sdf=True):
    """The stage on packs.  depth, sdf float32 [N], packed (depth non-decreasing inside a pack); pack_infos int64 [P, 2] = (first, len);
    u float32 [m] (one row of CDF positions for every pack) or [P, m] (per pack), non-decreasing, m >= 1.
    PRECONDITION: the packs tile [0, N) in order -- first_0 = 0, first_{p+1} = first_p + len_p, len_p >= 1 -- as the ``pack_infos`` of
    the hit rays of every marcher of this library do.  The layout of the outputs relies on it; it is not checked (that would be a
    host wait), and breaking it makes packs overlap in the outputs without any access leaving the buffers.
    -> (fine [P, m]: ``packed_sample_cdf`` of the pack's up-sampling CDF at u -- the opacity of ``neus_packed_sdf_to_alpha``, or of
    ``neus_packed_sdf_to_upsample_alpha`` with ``use_estimate``, through ``packed_alpha_to_vw`` and the normalised exclusive
    ``packed_cumsum``;
    merged [N + P m]: per pack the sorted union of depth and fine, pack p starting at first_p + p m, a new depth before an equal old one
    (``merge_two_packs_sorted_aligned``);
    sdf_merged [N + P m]: sdf at the old depths' places in merged; the places ``pidx_fine`` are left for the caller to fill;
    pidx_fine int64 [P, m]: the index in merged of every new depth;
    pack_infos_out int64 [P, 2] = (first_p + p m, len_p + m)).
    ``merge=False`` returns None for the last four (and needs no ``need_sdf``), ``need_sdf=False`` None for sdf_merged.
    Packs of any length are served: those with len + m <= PACKED_LDS_ROW in LDS, longer ones on global memory."""
    fine, _, merged, sdf_merged, _, pidx_fine, pack_infos_out = _stage_packed(
        "upsample_stage_packed", False, depth, sdf, None, pack_infos, u, inv_s, use_estimate, merge, need_sdf)
    return fine, merged, sdf_merged, pidx_fine, pack_infos_out


def upsample_stage_packed_blocks(depth, sdf, blidx, pack_infos, u, inv_s, use_estimate, merge=True, need_sdf=True):
    """``upsample_stage_packed`` on samples that carry a label each: blidx int64 [N], the block index of a forest's samples (any value,
    nothing interprets it).  Same arguments, precondition, entry point and kernel body otherwise.
    -> (fine, blidx_fine, merged, sdf_merged, blidx_merged, pidx_fine, pack_infos_out): fine, merged, sdf_merged, pidx_fine and
    pack_infos_out are the same bits as ``upsample_stage_packed`` returns on the same inputs;
    blidx_fine int64 [P, m]: the label of the upper end of the CDF bin every new depth was drawn from -- ``blidx[pidx]`` of
    ``packed_sample_cdf``'s second result -- taken before the new depth is raised to the running maximum;
    blidx_merged int64 [N + P m]: the labels in the order of merged -- an old depth keeps its label, ``blidx_merged[pidx_fine] ==
    blidx_fine``; None with ``merge=False``."""
    return _stage_packed("upsample_stage_packed_blocks", True, depth, sdf, blidx, pack_infos, u, inv_s, use_estimate, merge, need_sdf)
