"""nr3d_lib_amd.bindings._args -- the argument checks the ray-stage bindings share (``_neus_upsample``, ``_nerf_upsample``,
``_neus_alpha``, ``_neus_composite``).  Every failure is a RuntimeError that names the function and the argument."""
import torch

from .. import _hip as H


def chk(fn, name, t, shape=None, dtype=torch.float32):
    """``t`` is a contiguous GPU tensor of ``dtype`` and, when given, of ``shape``"""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{fn}: `{name}` must be a tensor, got {type(t).__name__}")
    H.require_gpu(t)
    if t.dtype != dtype:
        raise RuntimeError(f"{fn}: `{name}` must be {str(dtype).split('.')[-1]}, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{fn}: `{name}` must be {list(shape)}, got {list(t.shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"{fn}: `{name}` must be contiguous")
    return t


def same_device(fn, dev, first, **tensors):
    """every tensor given (None = absent) is on ``dev``, the device of the argument called ``first``"""
    for name, t in tensors.items():
        if t is not None and t.device != dev:
            raise RuntimeError(f"{fn}: `{name}` is on {t.device}, {first} on {dev}")


def u_rows(fn, u, rows):
    """the CDF positions: float32 [m], one row shared by all, or [rows, m], one each, m >= 1 -> (m, u_stride)"""
    chk(fn, "u", u)
    if u.dim() == 1 and u.shape[0] >= 1:
        return u.shape[0], 0
    if u.dim() == 2 and u.shape[0] == rows and u.shape[1] >= 1:
        return u.shape[1], u.shape[1]
    raise RuntimeError(f"{fn}: `u` must be [m] or [{rows}, m] with m >= 1, got {list(u.shape)}")
