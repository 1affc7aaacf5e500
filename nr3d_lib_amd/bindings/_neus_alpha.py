"""nr3d_lib_amd.bindings._neus_alpha -- the NeuS opacity of consecutive SDF samples, one launch each way (csrc/neus_alpha.hip through
include/nr3d_hip.h): ``alpha_i = max(0, (c_i - c_next) / (c_i + 1e-5))`` with ``c = sigmoid(sdf * inv_s)``, on packs and on rows.

Like ``_neus_upsample`` this module has NO reference twin: the reference runs the step as a chain of torch ops
(nr3d_lib/graphics/neus/neus_utils.py:48-117).  ``graphics.neus.neus_utils`` is its caller (``FUSED_SDF_TO_ALPHA``).
``inv_s`` is a Python number or a one-element float32 GPU tensor, which the kernels read on the device: no host wait either way.
A CPU tensor raises RuntimeError; there is no fallback here."""
import torch

from .. import _hip as H
from ._args import chk, same_device

__all__ = ["PACKED", "ROWS", "APPEND_NONE", "APPEND_ONE", "APPEND_SDF", "sdf_to_alpha_forward", "sdf_to_alpha_backward"]

PACKED, ROWS = 0, 1                              # NR3D_NEUS_ALPHA_PACKED / _ROWS
APPEND_NONE, APPEND_ONE, APPEND_SDF = 0, 1, 2    # NR3D_NEUS_ALPHA_APPEND_*


class _Call:
    """the arguments both directions share, checked: layout, sizes, append mode, inv_s as (value, device tensor | None)"""

    def __init__(self, fn, sdf, inv_s, pack_infos, append_cdf_1, pack_sdf_appends):
        chk(fn, "sdf", sdf)
        self.dev = dev = sdf.device
        if pack_infos is None:
            if sdf.dim() < 1 or sdf.shape[-1] < 1:
                raise RuntimeError(f"{fn}: `sdf` must be [..., n] with n >= 1, got {list(sdf.shape)}")
            if pack_sdf_appends is not None:
                raise RuntimeError(f"{fn}: `pack_sdf_appends` goes with `pack_infos` (rows take `append_cdf_1` only)")
            self.layout, self.n = ROWS, sdf.shape[-1]
            self.P, self.S = sdf.numel() // self.n, sdf.numel()
            self.ordered = 0
            n_out = self.n if append_cdf_1 else self.n - 1
            self.out_shape = (*sdf.shape[:-1], n_out)
        else:
            if sdf.dim() != 1:
                raise RuntimeError(f"{fn}: packed `sdf` must be [S], got {list(sdf.shape)}")
            chk(fn, "pack_infos", pack_infos, None, torch.int64)
            same_device(fn, dev, "sdf", pack_infos=pack_infos)
            if pack_infos.dim() != 2 or pack_infos.shape[1] != 2:
                raise RuntimeError(f"{fn}: `pack_infos` must be [P, 2], got {list(pack_infos.shape)}")
            self.layout, self.n = PACKED, 0
            self.P, self.S = pack_infos.shape[0], sdf.shape[0]
            self.ordered = 1 if (self.P > 0 and H.is_ordered(pack_infos)) else 0
            self.out_shape = (self.S,)
        if self.S >= 2 ** 32 or self.P >= 2 ** 32:
            raise RuntimeError(f"{fn}: {self.S} samples in {self.P} packs or rows, the limit is 2^32 - 1 each (split the batch)")
        if append_cdf_1:
            self.mode = APPEND_ONE                 # as the chain: append_cdf_1 overrides the appends
            pack_sdf_appends = None
        elif pack_sdf_appends is not None:
            chk(fn, "pack_sdf_appends", pack_sdf_appends, (self.P,))
            same_device(fn, dev, "sdf", pack_sdf_appends=pack_sdf_appends)
            self.mode = APPEND_SDF
        else:
            self.mode = APPEND_NONE
        self.appends = pack_sdf_appends
        if isinstance(inv_s, torch.Tensor):
            chk(fn, "inv_s", inv_s)
            same_device(fn, dev, "sdf", inv_s=inv_s)
            if inv_s.numel() != 1:
                raise RuntimeError(f"{fn}: `inv_s` must hold one element, got {list(inv_s.shape)}")
            self.inv_s, self.inv_s_dev = 0.0, inv_s
        else:
            self.inv_s, self.inv_s_dev = float(inv_s), None
        self.sdf, self.pack_infos = sdf, pack_infos

    def head(self):
        return (self.layout, self.P, self.S, self.n, H.ptr(self.sdf), H.ptr(self.pack_infos), self.mode, H.ptr(self.appends),
                self.inv_s, H.ptr(self.inv_s_dev), self.ordered)

    def out(self, shape):
        """an output over the samples: the ordered packs' kernel zeroes the rows outside the packs itself, the rows' kernels write
        every element; unordered packs write into zeros"""
        if self.layout == ROWS or self.ordered:
            return H.empty(shape, dtype=torch.float32, device=self.dev)
        return torch.zeros(shape, dtype=torch.float32, device=self.dev)


def sdf_to_alpha_forward(sdf, inv_s, pack_infos=None, append_cdf_1=False, pack_sdf_appends=None):
    """Rows (``pack_infos`` None): sdf float32 [..., n] -> alpha [..., n - 1], or [..., n] with ``append_cdf_1`` (a virtual last cdf of
    1).  Packed: sdf float32 [S], pack_infos int64 [P, 2] = (first, len) -> alpha [S]; the last sample of a pack closes an interval
    against 1 (``append_cdf_1``), against sigmoid(pack_sdf_appends[p] * inv_s) (``pack_sdf_appends`` float32 [P]) or has alpha 0; rows
    outside every pack are 0.  ``inv_s``: a Python number or a one-element float32 tensor on sdf's device."""
    c = _Call("sdf_to_alpha_forward", sdf, inv_s, pack_infos, append_cdf_1, pack_sdf_appends)
    if c.layout == PACKED and c.P == 0:
        return torch.zeros(c.out_shape, dtype=torch.float32, device=c.dev)
    alpha = c.out(c.out_shape)
    if alpha.numel():
        with H.on_device(c.dev):
            H.check(H.lib().nr3d_neus_alpha_fwd(*c.head(), H.ptr(alpha), H.stream_of(sdf)))
    return alpha


def sdf_to_alpha_backward(sdf, inv_s, grad_alpha, pack_infos=None, append_cdf_1=False, pack_sdf_appends=None, need_inv_s=False):
    """the gradients of ``sdf_to_alpha_forward`` from its inputs and ``grad_alpha`` (the forward's shape), recomputed, one launch:
    -> (dL/dsdf as sdf, 0 outside the packs; dL/dpack_sdf_appends [P] or None; dL/dinv_s float32 [1] or None).  ``need_inv_s`` adds
    the scalar: one partial per workgroup in a workspace, summed by a second launch of one workgroup -- written, the same bits run
    after run."""
    fn = "sdf_to_alpha_backward"
    c = _Call(fn, sdf, inv_s, pack_infos, append_cdf_1, pack_sdf_appends)
    chk(fn, "grad_alpha", grad_alpha, c.out_shape)
    same_device(fn, c.dev, "sdf", grad_alpha=grad_alpha)
    g_app = H.empty((c.P,), dtype=torch.float32, device=c.dev) if c.mode == APPEND_SDF else None
    if c.S == 0 or (c.layout == PACKED and c.P == 0) or grad_alpha.numel() == 0:      # no interval anywhere: nothing to launch
        return (torch.zeros_like(sdf), None if g_app is None else g_app.zero_(),
                torch.zeros(1, dtype=torch.float32, device=c.dev) if need_inv_s else None)
    g_sdf = c.out(sdf.shape)
    g_inv_s = H.empty((1,), dtype=torch.float32, device=c.dev) if need_inv_s else None
    with H.on_device(c.dev):
        l = H.lib()
        nbytes = int(l.nr3d_neus_alpha_bwd_workspace_bytes(c.layout, c.P, c.S)) if need_inv_s else 0
        ws = H.workspace(nbytes, c.dev) if need_inv_s else None
        H.check(l.nr3d_neus_alpha_bwd(*c.head(), H.ptr(grad_alpha), H.ptr(g_sdf), H.ptr(g_app), H.ptr(g_inv_s), H.ptr(ws), nbytes,
                                      H.stream_of(sdf)))
    return g_sdf, g_app, g_inv_s
