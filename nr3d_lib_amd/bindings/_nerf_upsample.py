"""nr3d_lib_amd.bindings._nerf_upsample -- the two packed stages of the NeRF march + up-sample ray query in one launch each
(csrc/nerf_upsample.hip through include/nr3d_hip.h): ``merge_rows_packs``, the union of every ray's coarse row with its marched pack,
and ``upsample_stage_packed``, one importance-resampling stage on the density.

Like ``_neus_upsample`` this module has NO reference twin: the reference runs both as chains of torch ops between two density queries
(nr3d_lib/graphics/nerf/nerf_ray_query.py:289-302 and :332-360).
``graphics.nerf.nerf_ray_query.nerf_ray_query_march_occ_multi_upsample_compressed`` is their caller.
A CPU tensor raises RuntimeError; there is no fallback here."""
import torch

from .. import _hip as H
from ._args import chk, same_device, u_rows

__all__ = ["LDS_ROW", "merge_rows_packs", "upsample_stage_packed"]


def __getattr__(name):
    """``LDS_ROW``: rows up to this many elements are staged in LDS (NR3D_NERF_UPSAMPLE_LDS_ROW), asked of the library so that it is
    stated once"""
    if name == "LDS_ROW":
        return int(H.lib().nr3d_nerf_upsample_lds_row())
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def merge_rows_packs(coarse, depth, pack_infos_all, rays_o, rays_d):
    """coarse float32 [R, nc] (non-decreasing per row, nc >= 1); depth float32 [N], the marched depths (non-decreasing inside a pack);
    pack_infos_all int64 [R, 2] = (first, len), the marched pack of EVERY ray in ray order: len 0 for a ray the marcher missed,
    first = the sum of the lengths before it (``get_pack_infos_from_n`` of the per-ray counts); rays_o, rays_d float32 [R, 3].
    -> (depths_all [R nc + N]: per ray the sorted union of its row and its pack; deltas_all: ``packed_diff`` of it, 0 at the end of a
    pack; ridx_all int64: the ray of every element; samples_all [R nc + N, 3] = ``torch.addcmul(o, d, t)``, bit for bit;
    pack_infos_out int64 [R, 2] = (r nc + first_r, nc + len_r)).
    Every output equals the op chain's (``merge_two_packs_sorted_a_includes_b`` -> index-puts -> addcmul -> ``packed_diff``) bit for
    bit.  Packs of any length are served: those with nc + len <= LDS_ROW in LDS, longer ones on global memory."""
    fn = "merge_rows_packs"
    chk(fn, "coarse", coarse)
    if coarse.dim() != 2 or coarse.shape[1] < 1:
        raise RuntimeError(f"{fn}: `coarse` must be [R, nc] with nc >= 1, got {list(coarse.shape)}")
    R, nc = coarse.shape
    chk(fn, "depth", depth)
    if depth.dim() != 1:
        raise RuntimeError(f"{fn}: `depth` must be [N], got {list(depth.shape)}")
    N = depth.shape[0]
    chk(fn, "pack_infos_all", pack_infos_all, (R, 2), torch.int64)
    chk(fn, "rays_o", rays_o, (R, 3))
    chk(fn, "rays_d", rays_d, (R, 3))
    dev = coarse.device
    same_device(fn, dev, "coarse", depth=depth, pack_infos_all=pack_infos_all, rays_o=rays_o, rays_d=rays_d)
    total = R * nc + N
    if total >= 2 ** 31:
        raise RuntimeError(f"{fn}: R nc + N = {total}, the merged buffer holds at most 2^31 - 1 elements (split the batch)")
    if R == 0:
        total = 0            # no ray owns a marched sample
    depths_all = H.empty((total,), dtype=torch.float32, device=dev)
    deltas_all = H.empty((total,), dtype=torch.float32, device=dev)
    ridx_all = H.empty((total,), dtype=torch.int64, device=dev)
    samples_all = H.empty((total, 3), dtype=torch.float32, device=dev)
    pack_infos_out = H.empty((R, 2), dtype=torch.int64, device=dev)
    if R:
        with H.on_device(dev):
            H.check(H.lib().nr3d_nerf_merge_rows_packs(R, nc, N, H.ptr(coarse), H.ptr(depth), H.ptr(pack_infos_all), H.ptr(rays_o),
                                                       H.ptr(rays_d), H.ptr(depths_all), H.ptr(deltas_all), H.ptr(ridx_all),
                                                       H.ptr(samples_all), H.ptr(pack_infos_out), H.stream_of(coarse)))
    return depths_all, deltas_all, ridx_all, samples_all, pack_infos_out


def upsample_stage_packed(depth, sigma, delta, pack_infos, u, coarse=None, coarse_row=None):
    """The stage on packs.  depth, sigma, delta float32 [N], packed (depth non-decreasing inside a pack); pack_infos int64 [P, 2] =
    (first, len); u float32 [m] (one row of CDF positions for every pack) or [P, m] (per pack), non-decreasing, m = num_fine + 1 >= 1.
    PRECONDITION: the packs tile [0, N) in order -- first_0 = 0, first_{p+1} = first_p + len_p, len_p >= 1 -- as for
    ``_neus_upsample.upsample_stage_packed``; it is not checked (that would be a host wait), and breaking it makes packs share elements
    without any access leaving the buffers.
    coarse (optional) float32 [Rc, nc], non-decreasing per row, with coarse_row int64 [P]: the row that belongs to pack p (None: row
    p, then Rc == P).
    -> (fine [P, m]: ``packed_sample_cdf`` at u of the pack's CDF -- the inclusive ``packed_cumsum`` of ``1 - exp(-sigma delta)``
    divided by max(its last value, 1e-5), the opacity evaluated as ``-expm1(-sigma delta)`` -- raised to its running maximum along the
    row (the reference sorts the row instead);
    with coarse: merged [P, nc + m], the sorted union of the coarse row and fine, and deltas [P, nc + m], ``packed_diff`` of it (last
    column 0); without: merged [P, m - 1] = fine[:, :-1] + deltas and deltas [P, m - 1] = fine.diff(dim=-1)).
    Packs of any length are served: those with len + m + nc <= LDS_ROW in LDS, longer ones on global memory."""
    fn = "upsample_stage_packed"
    chk(fn, "depth", depth)
    if depth.dim() != 1:
        raise RuntimeError(f"{fn}: `depth` must be [N], got {list(depth.shape)}")
    N = depth.shape[0]
    chk(fn, "sigma", sigma, (N,))
    chk(fn, "delta", delta, (N,))
    chk(fn, "pack_infos", pack_infos, None, torch.int64)
    if pack_infos.dim() != 2 or pack_infos.shape[1] != 2:
        raise RuntimeError(f"{fn}: `pack_infos` must be [P, 2], got {list(pack_infos.shape)}")
    P = pack_infos.shape[0]
    m, u_stride = u_rows(fn, u, P)
    nc = n_rows = 0
    if coarse is None:
        if coarse_row is not None:
            raise RuntimeError(f"{fn}: `coarse_row` without `coarse`")
    else:
        chk(fn, "coarse", coarse)
        if coarse.dim() != 2 or coarse.shape[1] < 1:
            raise RuntimeError(f"{fn}: `coarse` must be [Rc, nc] with nc >= 1, got {list(coarse.shape)}")
        n_rows, nc = coarse.shape
        if coarse_row is not None:
            chk(fn, "coarse_row", coarse_row, (P,), torch.int64)
        elif n_rows != P:
            raise RuntimeError(f"{fn}: `coarse` must be [{P}, nc] without `coarse_row`, got {list(coarse.shape)}")
        if P and n_rows == 0:
            raise RuntimeError(f"{fn}: `coarse` has no rows for {P} packs")
    dev = depth.device
    same_device(fn, dev, "depth", sigma=sigma, delta=delta, pack_infos=pack_infos, u=u, coarse=coarse, coarse_row=coarse_row)
    if N >= 2 ** 31 or P * (m + nc) >= 2 ** 31:
        raise RuntimeError(f"{fn}: N = {N}, P (m + nc) = {P * (m + nc)}: at most 2^31 - 1 elements each (split the batch)")
    width = nc + m if nc else m - 1
    fine = H.empty((P, m), dtype=torch.float32, device=dev)
    merged = H.empty((P, width), dtype=torch.float32, device=dev)
    deltas = H.empty((P, width), dtype=torch.float32, device=dev)
    if P:
        workspace = H.empty((max(N, 1),), dtype=torch.float32, device=dev)       # the CDF of the packs that do not fit the LDS row
        with H.on_device(dev):
            H.check(H.lib().nr3d_nerf_upsample_stage_packed(P, N, m, nc, n_rows, H.ptr(depth), H.ptr(sigma), H.ptr(delta),
                                                            H.ptr(pack_infos), H.ptr(u), u_stride, H.ptr(coarse), H.ptr(coarse_row),
                                                            H.ptr(workspace), H.ptr(fine), H.ptr(merged), H.ptr(deltas),
                                                            H.stream_of(depth)))
    return fine, merged, deltas
