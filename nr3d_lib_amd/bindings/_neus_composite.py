"""nr3d_lib_amd.bindings._neus_composite -- the last stage of a NeuS render, one launch each way (csrc/neus_composite.hip through
include/nr3d_hip.h): the volume buffer's ``alpha, t, rgb, nablas`` -> ``vw, mask, depth, rgb, normals``, on rows ('batched' buffers) and
on packs.

Like ``_neus_alpha`` this module has NO reference twin: the reference runs the step as a chain of torch ops
(nr3d_lib/models/fields/neus/renderer_mixin.py:396-439).  ``graphics.neus.neus_render`` is its caller (``FUSED_NEUS_COMPOSITE``).
A CPU tensor raises RuntimeError; there is no fallback here."""
import torch

from .. import _hip as H
from ._args import chk, same_device

__all__ = ["ROWS", "PACKED", "NORMALS_RAW", "NORMALS_UNIT", "neus_composite_forward", "neus_composite_backward"]

ROWS, PACKED = 0, 1                     # NR3D_NEUS_COMPOSITE_ROWS / _PACKED
NORMALS_RAW, NORMALS_UNIT = 0, 1        # normals_mode: sum w nablas | sum w normalize(clamp(nablas, -1, 1)), nablas clamped in place


def _on(fn, dev, name, t, shape, dtype=torch.float32):
    chk(fn, name, t, shape, dtype)
    same_device(fn, dev, "alphas", **{name: t})


class _Call:
    """the arguments both directions share, checked: layout, sizes, the per-sample inputs, the scatter index"""

    def __init__(self, fn, alphas, t, rgb, nablas, pack_infos, rays_inds_hit, num_rays, early_stop_eps, alpha_thre, normalize_depth,
                 normals_mode):
        if not isinstance(alphas, torch.Tensor):
            raise RuntimeError(f"{fn}: `alphas` must be a tensor, got {type(alphas).__name__}")
        if pack_infos is None:
            if alphas.dim() != 2 or alphas.shape[1] < 1:
                raise RuntimeError(f"{fn}: rows need `alphas` [R, n] with n >= 1, got {list(alphas.shape)}")
            self.layout, self.P, self.n = ROWS, alphas.shape[0], alphas.shape[1]
        else:
            if alphas.dim() != 1:
                raise RuntimeError(f"{fn}: packed `alphas` must be [S], got {list(alphas.shape)}")
            self.layout, self.P, self.n = PACKED, pack_infos.shape[0] if pack_infos.dim() else -1, 0
        self.shape, self.S = tuple(alphas.shape), alphas.numel()
        chk(fn, "alphas", alphas, self.shape)
        self.dev = dev = alphas.device
        if pack_infos is not None:
            _on(fn, dev, "pack_infos", pack_infos, (max(self.P, 0), 2), torch.int64)
        _on(fn, dev, "t", t, self.shape)
        if rgb is not None:
            _on(fn, dev, "rgb", rgb, (*self.shape, 3))
        if nablas is not None:
            _on(fn, dev, "nablas", nablas, (*self.shape, 3))
        if self.S >= 2 ** 32 or self.P >= 2 ** 32:
            raise RuntimeError(f"{fn}: {self.S} samples in {self.P} packs or rows, the limit is 2^32 - 1 each (split the batch)")
        if normals_mode not in (NORMALS_RAW, NORMALS_UNIT):
            raise RuntimeError(f"{fn}: normals_mode = {normals_mode!r}, must be 0 (raw) or 1 (clamped and normalised)")
        if rays_inds_hit is not None:
            _on(fn, dev, "rays_inds_hit", rays_inds_hit, (self.P,), torch.int64)
            self.num_rays = int(num_rays)
        else:
            if num_rays is not None and int(num_rays) != self.P:
                raise RuntimeError(f"{fn}: num_rays = {num_rays} must equal the number of rows or packs ({self.P}) when rays_inds_hit is None")
            self.num_rays = self.P
        self.alphas, self.t, self.rgb, self.nablas = alphas, t, rgb, nablas
        self.pack_infos, self.rays_inds_hit = pack_infos, rays_inds_hit
        self.tail = (float(early_stop_eps), float(alpha_thre), 1 if normalize_depth else 0, int(normals_mode))

    def head(self):
        return (self.layout, self.P, self.S, self.n, H.ptr(self.alphas), H.ptr(self.t), H.ptr(self.rgb), H.ptr(self.nablas),
                H.ptr(self.pack_infos), H.ptr(self.rays_inds_hit), *self.tail)

    def per_sample(self, inner, packs_tile):
        """an output over the samples: the kernels write every sample of a row or pack; samples outside every pack are zeros unless the
        caller states that the packs tile [0, S)"""
        shape = self.shape if inner is None else (*self.shape, inner)
        full = self.P > 0 and (self.layout == ROWS or packs_tile)
        return (H.empty if full else torch.zeros)(shape, dtype=torch.float32, device=self.dev)

    def per_ray(self, inner=None):
        """zeros where the results are scattered (rays that are not hit stay zero), else every element is written"""
        shape = (self.num_rays,) if inner is None else (self.num_rays, inner)
        scattered = self.rays_inds_hit is not None or self.P == 0
        return (torch.zeros if scattered else H.empty)(shape, dtype=torch.float32, device=self.dev)


def neus_composite_forward(alphas, t, rgb=None, nablas=None, pack_infos=None, rays_inds_hit=None, num_rays=None, early_stop_eps=1e-4,
                           alpha_thre=0.0, normalize_depth=True, normals_mode=NORMALS_RAW, packs_tile=False):
    """Rows (``pack_infos`` None): alphas, t float32 [R, n]; rgb, nablas [R, n, 3] | None; ``early_stop_eps`` / ``alpha_thre`` unused.
    Packed: alphas, t [S]; rgb, nablas [S, 3] | None; pack_infos int64 [P, 2] = (first, len).  rays_inds_hit int64 [R | P] | None scatters
    the per-ray results into [num_rays] outputs.  ``normals_mode`` 1 clamps ``nablas`` IN PLACE to [-1, 1] and composites the unit vectors.
    -> (vw as alphas, mask [num_rays], depth [num_rays], rgb_out [num_rays, 3] | None, normals_out [num_rays, 3] | None)"""
    fn = "neus_composite_forward"
    c = _Call(fn, alphas, t, rgb, nablas, pack_infos, rays_inds_hit, num_rays, early_stop_eps, alpha_thre, normalize_depth, normals_mode)
    with H.on_device(c.dev):
        vw = c.per_sample(None, packs_tile)
        mask, depth = c.per_ray(), c.per_ray()
        rgb_out = c.per_ray(3) if rgb is not None else None
        normals_out = c.per_ray(3) if nablas is not None else None
        if c.P > 0:
            H.check(H.lib().nr3d_neus_composite_fwd(*c.head(), H.ptr(vw), H.ptr(mask), H.ptr(depth), H.ptr(rgb_out), H.ptr(normals_out),
                                                    H.stream_of(alphas)))
    return vw, mask, depth, rgb_out, normals_out


def neus_composite_backward(alphas, t, rgb, nablas, pack_infos, rays_inds_hit, early_stop_eps, alpha_thre, normalize_depth, normals_mode,
                            vw, mask, depth, g_mask, g_depth, g_rgb, g_normals, g_vw, need_t=True, need_rgb=True, need_nablas=True,
                            packs_tile=False):
    """the gradients of ``neus_composite_forward`` in one launch; ``vw, mask, depth`` are its outputs, the ``g_*`` the grads of its
    outputs (None = zero).  -> (grad_alphas, grad_t | None, grad_rgb | None, grad_nablas | None), shaped as the inputs.
    ``normals_mode`` 1 with ``g_normals`` or a wanted ``grad_nablas`` is refused by the library: the normalised normals are forward only."""
    fn = "neus_composite_backward"
    c = _Call(fn, alphas, t, rgb, nablas, pack_infos, rays_inds_hit, mask.shape[0] if isinstance(mask, torch.Tensor) else None,
              early_stop_eps, alpha_thre, normalize_depth, normals_mode)
    nr, dev = c.num_rays, c.dev
    _on(fn, dev, "vw", vw, c.shape)
    for name, g, shape in (("mask", mask, (nr,)), ("depth", depth, (nr,)), ("g_mask", g_mask, (nr,)), ("g_depth", g_depth, (nr,)),
                           ("g_rgb", g_rgb, (nr, 3)), ("g_normals", g_normals, (nr, 3)), ("g_vw", g_vw, c.shape)):
        if g is not None or name in ("mask", "depth"):
            _on(fn, dev, name, g, shape)
    with H.on_device(dev):
        ga = c.per_sample(None, packs_tile)
        gt = c.per_sample(None, packs_tile) if need_t else None
        gr = c.per_sample(3, packs_tile) if (need_rgb and rgb is not None) else None
        gn = c.per_sample(3, packs_tile) if (need_nablas and nablas is not None) else None
        if c.P > 0:
            H.check(H.lib().nr3d_neus_composite_bwd(*c.head(), H.ptr(vw), H.ptr(mask), H.ptr(depth), H.ptr(g_mask), H.ptr(g_depth),
                                                    H.ptr(g_rgb), H.ptr(g_normals), H.ptr(g_vw), H.ptr(ga), H.ptr(gt), H.ptr(gr), H.ptr(gn),
                                                    H.stream_of(alphas)))
    return ga, gt, gr, gn
