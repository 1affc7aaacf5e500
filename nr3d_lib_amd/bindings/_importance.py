"""nr3d_lib_amd.bindings._importance -- pixel importance sampling on accumulated error maps (csrc/importance.hip through
include/nr3d_hip.h): the inverse-CDF sampler of one or several maps in one launch, the accumulating and reproducible bilinear update
of a map, and the three CDFs of a map by wave-row scans in a fixed order.

This module has NO reference twin: the reference runs all three as chains of torch ops (nr3d_lib/models/importance.py).
``models.importance`` is its caller (``FUSED_IMPORTANCE``).  A CPU tensor raises RuntimeError; there is no fallback here."""
import ctypes as C

import torch

from .. import _hip as H
from ._args import chk, same_device

__all__ = ["MAX_MAPS", "UPDATE_CHUNK", "FRAME_SAMPLED", "FRAME_CONST", "FRAME_TENSOR", "sample", "update", "construct_cdf"]

MAX_MAPS = 8                                          # NR3D_IMPORTANCE_MAX_MAPS
UPDATE_CHUNK = 2 ** 15                                # NR3D_IMPORTANCE_UPDATE_CHUNK
FRAME_SAMPLED, FRAME_CONST, FRAME_TENSOR = 0, 1, 2    # NR3D_IMPORTANCE_FRAME_*


class _CMap(C.Structure):
    _fields_ = [("cdf_img", C.c_void_p), ("cdf_y", C.c_void_p), ("cdf_x_cond_y", C.c_void_p),
                ("res_y", C.c_uint32), ("res_x", C.c_uint32), ("first", C.c_uint32), ("reserved", C.c_uint32)]


def sample(maps, firsts, n_uniform, n_images, u_img, u_x, u_y, frame_ind=None, need_i=True, need_xy=True):
    """``maps``: up to 8 triples (cdf_img [N] | None, cdf_y [N, H], cdf_x_cond_y [N, H, W]) of float32 GPU tensors; ``firsts``: the first
    sample of each map's segment (non-decreasing, firsts[0] == n_uniform); samples [0, n_uniform) are uniform.  ``u_img``, ``u_x``,
    ``u_y``: float32 [n] each; u_img may be None with a given ``frame_ind`` (an int, or int64 [n]), u_x and u_y without ``need_xy``.
    -> (i int64 [n] | None, xy float32 [n, 2] | None)"""
    fn = "importance.sample"
    first_u = next((t for t in (u_img, u_x, u_y) if t is not None), None)
    if first_u is None:
        raise RuntimeError(f"{fn}: no uniforms")
    chk(fn, "u", first_u)
    dev, n = first_u.device, first_u.numel()
    for name, t, needed in (("u_img", u_img, frame_ind is None), ("u_x", u_x, need_xy), ("u_y", u_y, need_xy)):
        if t is not None or needed:
            chk(fn, name, t, (n,))
            same_device(fn, dev, "u", **{name: t})
    if n >= 2 ** 32:
        raise RuntimeError(f"{fn}: {n} samples, the limit is 2^32 - 1")
    if len(maps) > MAX_MAPS or len(maps) != len(firsts):
        raise RuntimeError(f"{fn}: {len(maps)} maps with {len(firsts)} segments, at most {MAX_MAPS} of each and as many of one as of the other")
    table = (_CMap * max(len(maps), 1))()
    for k, ((cdf_img, cdf_y, cdf_x), first) in enumerate(zip(maps, firsts)):
        if frame_ind is None or cdf_img is not None:
            chk(fn, f"maps[{k}].cdf_img", cdf_img, (n_images,))
        chk(fn, f"maps[{k}].cdf_y", cdf_y)
        if cdf_y.dim() != 2 or cdf_y.shape[0] != n_images or cdf_y.shape[1] < 1:
            raise RuntimeError(f"{fn}: `maps[{k}].cdf_y` must be [{n_images}, H], got {list(cdf_y.shape)}")
        chk(fn, f"maps[{k}].cdf_x_cond_y", cdf_x)
        if cdf_x.dim() != 3 or tuple(cdf_x.shape[:2]) != tuple(cdf_y.shape) or cdf_x.shape[2] < 1:
            raise RuntimeError(f"{fn}: `maps[{k}].cdf_x_cond_y` must be [{n_images}, {cdf_y.shape[1]}, W], got {list(cdf_x.shape)}")
        same_device(fn, dev, "u", cdf_img=cdf_img, cdf_y=cdf_y, cdf_x_cond_y=cdf_x)
        table[k] = _CMap(H.ptr(cdf_img), H.ptr(cdf_y), H.ptr(cdf_x), cdf_y.shape[1], cdf_x.shape[2], int(first), 0)
    mode, f_const, f_dev = FRAME_SAMPLED, 0, None
    if isinstance(frame_ind, torch.Tensor):
        chk(fn, "frame_ind", frame_ind, (n,), torch.int64)
        same_device(fn, dev, "u", frame_ind=frame_ind)
        mode, f_dev = FRAME_TENSOR, frame_ind
    elif frame_ind is not None:
        mode, f_const = FRAME_CONST, int(frame_ind)
        if not -n_images <= f_const < n_images:
            raise IndexError(f"{fn}: frame {f_const} of {n_images} images")
    out_i = H.empty((n,), dtype=torch.int64, device=dev) if need_i else None
    out_xy = H.empty((n, 2), dtype=torch.float32, device=dev) if need_xy else None
    if n and (need_i or need_xy):
        with H.on_device(dev):
            H.check(H.lib().nr3d_importance_sample(n, int(n_images), int(n_uniform), len(maps), table, H.ptr(u_img), H.ptr(u_x), H.ptr(u_y),
                                                   mode, f_const, H.ptr(f_dev), H.ptr(out_i), H.ptr(out_xy), H.stream_of(first_u)))
    return out_i, out_xy


def update(error_map, acc, frame_ind, xy, val):
    """error_map float32 [N, H, W] += the bilinear splat of val [n] at xy [n, 2] of frame ``frame_ind`` (int, or int64 [n]); ``acc``:
    int64 [N, H, W], all zero, and all zero again afterwards.  Calls of more than 2^15 samples go in chunks of 2^15, in order."""
    fn = "importance.update"
    chk(fn, "error_map", error_map)
    if error_map.dim() != 3:
        raise RuntimeError(f"{fn}: `error_map` must be [N, H, W], got {list(error_map.shape)}")
    dev = error_map.device
    chk(fn, "acc", acc, error_map.shape, torch.int64)
    chk(fn, "val", val)
    n = val.numel()
    val = val.reshape(n)
    chk(fn, "xy", xy)
    if xy.numel() != 2 * n or xy.shape[-1] != 2:
        raise RuntimeError(f"{fn}: `xy` must be [..., 2] with val's prefix {list(val.shape)}, got {list(xy.shape)}")
    xy = xy.reshape(n, 2)
    f_const, f_dev = 0, None
    if isinstance(frame_ind, torch.Tensor):
        chk(fn, "frame_ind", frame_ind, None, torch.int64)
        if frame_ind.numel() != n:
            raise RuntimeError(f"{fn}: `frame_ind` must hold {n} frames, got {list(frame_ind.shape)}")
        f_dev = frame_ind.reshape(n)
    else:
        f_const = int(frame_ind)
    same_device(fn, dev, "error_map", acc=acc, xy=xy, val=val, frame_ind=f_dev)
    N, Hh, W = error_map.shape
    with H.on_device(dev):
        l, st = H.lib(), H.stream_of(error_map)
        for b in range(0, n, UPDATE_CHUNK):
            m = min(UPDATE_CHUNK, n - b)
            H.check(l.nr3d_importance_update(m, N, Hh, W, f_const, H.ptr(f_dev[b:]) if f_dev is not None else None, H.ptr(xy[b:]),
                                             H.ptr(val[b:]), H.ptr(error_map), H.ptr(acc), st))


def construct_cdf(error_map, min_pdf, max_pdf=None, clean=False):
    """-> (cdf_x_cond_y [N, H, W], cdf_y [N, H], cdf_img [N]) of error_map float32 [N, H, W]; the map is clamped to ``max_pdf`` in place
    when that is given, and zeroed with ``clean``.  ``1 - min_pdf`` is taken in Python's double and rounded once."""
    fn = "importance.construct_cdf"
    chk(fn, "error_map", error_map)
    if error_map.dim() != 3 or error_map.numel() == 0:
        raise RuntimeError(f"{fn}: `error_map` must be a non-empty [N, H, W], got {list(error_map.shape)}")
    dev = error_map.device
    N, Hh, W = error_map.shape
    cdf_x = H.empty((N, Hh, W), dtype=torch.float32, device=dev)
    cdf_y = H.empty((N, Hh), dtype=torch.float32, device=dev)
    cdf_img = H.empty((N,), dtype=torch.float32, device=dev)
    ws = H.empty((N * Hh + N,), dtype=torch.float32, device=dev)
    with H.on_device(dev):
        H.check(H.lib().nr3d_importance_construct_cdf(N, Hh, W, H.ptr(error_map), float(1 - min_pdf), float(min_pdf), int(max_pdf is not None),
                                                      float(max_pdf) if max_pdf is not None else 0.0, int(bool(clean)), H.ptr(cdf_x),
                                                      H.ptr(cdf_y), H.ptr(cdf_img), H.ptr(ws), H.ptr(ws[N * Hh:]), H.stream_of(error_map)))
    return cdf_x, cdf_y, cdf_img
