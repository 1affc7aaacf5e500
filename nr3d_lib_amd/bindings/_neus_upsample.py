"""nr3d_lib_amd.bindings._neus_upsample -- one up-sampling stage of the vanilla NeuS coarse ray query in one launch
(csrc/neus_upsample.hip through include/nr3d_hip.h).

Like ``_mlp`` this module has NO reference twin: the reference runs a stage as a chain of torch ops between two SDF queries
(nr3d_lib/graphics/neus/neus_ray_query.py:258-270).  ``graphics.neus.neus_ray_query.neus_ray_query_coarse_multi_upsample`` is its
caller.  A CPU tensor raises RuntimeError; there is no fallback here."""
import torch

from .. import _hip as H

__all__ = ["MAX_ROW", "upsample_stage"]


def __getattr__(name):
    """``MAX_ROW``: the library's cap on n + m (NR3D_NEUS_UPSAMPLE_MAX_ROW), asked of the library so that it is stated once"""
    if name == "MAX_ROW":
        return int(H.lib().nr3d_neus_upsample_max_row())
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _chk(name, t, shape):
    fn = "upsample_stage"
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{fn}: `{name}` must be a tensor, got {type(t).__name__}")
    H.require_gpu(t)
    if t.dtype != torch.float32:
        raise RuntimeError(f"{fn}: `{name}` must be float32, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{fn}: `{name}` must be {list(shape)}, got {list(t.shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"{fn}: `{name}` must be contiguous")
    return t


def upsample_stage(depth, sdf, u, inv_s, use_estimate):
    """depth, sdf float32 [R, n] (depth non-decreasing per row, n >= 2); u float32 [m] (one row of CDF positions for every ray) or
    [R, m] (per ray), non-decreasing, m >= 1; n + m <= MAX_ROW.
    -> (fine [R, m]: the inverse of the row's up-sampling CDF at u, non-decreasing; merged [R, n + m]: the sorted union of depth and
    fine; order int32 [R, n + m]: merged == cat([depth, fine], -1).gather(-1, order), depth elements first on equal values).
    ``use_estimate``: the NeuS paper's slope estimate (neus_ray_sdf_to_upsample_alpha) instead of neus_ray_sdf_to_alpha."""
    fn = "upsample_stage"
    _chk("depth", depth, None)
    if depth.dim() != 2 or depth.shape[1] < 2:
        raise RuntimeError(f"{fn}: `depth` must be [R, n] with n >= 2, got {list(depth.shape)}")
    R, n = depth.shape
    _chk("sdf", sdf, (R, n))
    _chk("u", u, None)
    if u.dim() == 1 and u.shape[0] >= 1:
        m, u_stride = u.shape[0], 0
    elif u.dim() == 2 and u.shape[0] == R and u.shape[1] >= 1:
        m, u_stride = u.shape[1], u.shape[1]
    else:
        raise RuntimeError(f"{fn}: `u` must be [m] or [{R}, m] with m >= 1, got {list(u.shape)}")
    dev = depth.device
    for name, t in (("sdf", sdf), ("u", u)):
        if t.device != dev:
            raise RuntimeError(f"{fn}: `{name}` is on {t.device}, depth on {dev}")
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
