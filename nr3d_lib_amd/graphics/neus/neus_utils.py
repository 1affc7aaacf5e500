"""NeuS opacity from SDF samples -- counterpart of nr3d_lib/graphics/neus/neus_utils.py:48-217 (same names, arguments and return
conventions).  Alpha of the interval between two consecutive samples = relative drop of the logistic CDF
``sigmoid(sdf * inv_s)``; packed variants take the difference inside each pack (last sample: appended value or 0).
(The reference's ``neus_packed_sdf_to_vw`` calls ``packed_alpha_to_vw`` without its ``pack_infos`` (:115) and its
``neus_packed_sdf_to_tau`` tests a tensor for truth (:103); here the pack_infos are passed and the test is ``is not None``.)"""
from typing import Union

import torch
import torch.nn.functional as F

from nr3d_lib_amd.bindings import _neus_alpha as _backend
from nr3d_lib_amd.graphics.nerf.nerf_utils import ray_alpha_to_vw
from nr3d_lib_amd.graphics.pack_ops import packed_alpha_to_vw, packed_diff

__all__ = ['neus_pdf', 'neus_cdf', 'neus_ray_cdf_to_alpha', 'neus_ray_sdf_to_tau', 'neus_ray_sdf_to_alpha', 'neus_ray_sdf_to_vw',
           'neus_packed_cdf_to_alpha', 'neus_packed_sdf_to_tau', 'neus_packed_sdf_to_alpha', 'neus_packed_sdf_to_vw',
           'neus_estimate_sdf_nablas_to_alpha', 'neus_packed_sdf_to_upsample_alpha', 'neus_ray_sdf_to_upsample_alpha']


# neus_ray_sdf_to_alpha / neus_packed_sdf_to_alpha (and the _vw helpers on top of them): True = one launch of the HIP kernel each way
# (bindings._neus_alpha) for a float32 GPU sdf with a scalar inv_s; False (and every other input) = the reference's torch op chain.
# Same semantics.  A call's own ``fused=False`` always takes the chain.
FUSED_SDF_TO_ALPHA = True


def neus_pdf(x: torch.Tensor, inv_s):
    """logistic density with scale 1 / inv_s, the cosh clamped to [-20, 20] (maths/common.py:109-120)"""
    return 0.25 * inv_s / (torch.cosh(inv_s * x / 2.).clamp(-20, 20) ** 2)


def neus_cdf(x, inv_s):
    return torch.sigmoid(x * inv_s)


def neus_ray_cdf_to_alpha(cdf: torch.Tensor, append_cdf_1=False):
    """[..., n] cdf -> [..., n-1] alpha (or [..., n] with a virtual last cdf of 1)"""
    if append_cdf_1:
        drop, ref = -cdf.diff(append=cdf.new_ones((*cdf.shape[:-1], 1))), cdf
    else:
        drop, ref = -cdf.diff(), cdf[..., :-1]
    return (drop / (ref + 1e-5)).clamp_min(0)


class _SdfToAlpha(torch.autograd.Function):
    """alpha of consecutive SDF samples as one kernel each way (the chain below: 7 launches forward and 25 backward in eager
    PyTorch with a learnable inv_s, profiles/neus_alpha.json).  Only sdf, inv_s and the appends are kept; the backward recomputes the rest.  ``layout`` = (pack_infos | None,
    append_cdf_1): not tensors for autograd, so pack_infos keeps its ``mark_ordered`` tag."""

    @staticmethod
    def forward(ctx, sdf, inv_s, appends, layout):
        ctx.layout = layout
        ctx.inv_s = None if isinstance(inv_s, torch.Tensor) else inv_s
        ctx.save_for_backward(sdf, inv_s if ctx.inv_s is None else None, appends)
        return _backend.sdf_to_alpha_forward(sdf, inv_s, layout[0], layout[1], appends)

    @staticmethod
    def backward(ctx, grad_alpha):
        sdf, inv_s_t, appends = ctx.saved_tensors
        inv_s = inv_s_t if ctx.inv_s is None else ctx.inv_s
        pack_infos, append_cdf_1 = ctx.layout
        need = ctx.needs_input_grad
        if torch.is_grad_enabled():
            # create_graph=True: a higher-order graph is wanted -> the gradient as differentiable torch ops on the saved inputs: the
            # autograd of the chain's own ops (rows) or of their restatement by indexing (packs: the chain's packed_diff is
            # differentiable once); first-order training never takes this branch
            wrt = [t for t, n in zip((sdf, inv_s_t, appends), need) if n]
            with torch.enable_grad():
                alpha = (neus_ray_cdf_to_alpha(neus_cdf(sdf, inv_s), append_cdf_1) if pack_infos is None else
                         _packed_sdf_to_alpha_by_index(sdf, inv_s, pack_infos, append_cdf_1, appends))
                got = iter(torch.autograd.grad(alpha, wrt, grad_alpha, create_graph=True, allow_unused=True))
            return tuple(next(got) if n else None for n in need[:3]) + (None,)
        g_sdf, g_app, g_inv_s = _backend.sdf_to_alpha_backward(sdf, inv_s, grad_alpha.contiguous(), pack_infos, append_cdf_1, appends,
                                                               need_inv_s=need[1])
        return (g_sdf if need[0] else None, g_inv_s.reshape(inv_s_t.shape) if need[1] else None,
                g_app if need[2] else None, None)


def _packed_sdf_to_alpha_by_index(sdf, inv_s, pack_infos, append_cdf_1, appends):
    """neus_packed_sdf_to_alpha in torch ops that can be differentiated twice, without a host wait: c_next by a shift, the packs'
    last samples and the rows outside the packs by scattered marks (packs in any order, with gaps, of any length)"""
    S = sdf.shape[0]
    first, lens = pack_infos[:, 0], pack_infos[:, 1]
    some = lens > 0
    cdf = neus_cdf(sdf, inv_s)
    if S == 0:
        return cdf
    edges = torch.zeros(S + 1, dtype=torch.int32, device=sdf.device)
    edges.index_add_(0, first, some.int()).index_add_(0, first + lens, -some.int())
    in_pack = edges.cumsum(0)[:S] > 0
    at = (first + lens - 1).clamp(0, max(S - 1, 0))
    is_last = torch.zeros(S, dtype=torch.int32, device=sdf.device).index_add_(0, at, some.int()) > 0
    if append_cdf_1:
        tail = cdf.new_ones(S)
    elif appends is not None:
        tail = cdf.new_zeros(S).index_add(0, at, torch.where(some, neus_cdf(appends, inv_s), cdf.new_zeros(())))
    else:
        tail = None
    c_next = torch.where(is_last, tail if tail is not None else cdf, cdf.roll(-1))
    closes = in_pack if tail is not None else in_pack & ~is_last
    return (torch.where(closes, cdf - c_next, cdf.new_zeros(())) / (cdf + 1e-5)).clamp_min(0)


def _fused_sdf_to_alpha(fused, sdf, inv_s, pack_infos, append_cdf_1, appends):
    """alpha through the kernel, or None when the chain has to run: the switch (or the call) is off, or the inputs are not a float32
    GPU sdf with inv_s a Python number, a one-element CPU tensor without grad or a one-element float32 GPU tensor.  Only the route
    is decided here; shapes, devices and the other dtypes are the binding's to check (it raises)."""
    if not (FUSED_SDF_TO_ALPHA if fused is None else fused):
        return None
    if not (isinstance(sdf, torch.Tensor) and sdf.is_cuda and sdf.dtype == torch.float32):
        return None
    if isinstance(inv_s, torch.Tensor):
        if inv_s.numel() != 1 or (inv_s.is_cuda and inv_s.dtype != torch.float32) or (not inv_s.is_cuda and inv_s.requires_grad):
            return None
        if not inv_s.is_cuda:
            inv_s = float(inv_s.item())             # host memory: no device wait
    elif isinstance(inv_s, bool) or not isinstance(inv_s, (int, float)):
        return None
    if append_cdf_1 or pack_infos is None:
        appends = None                              # as the chain: append_cdf_1 overrides the appends; rows have none
    elif appends is not None:
        appends = appends.contiguous()
    sdf = sdf.contiguous()
    if pack_infos is not None:
        pack_infos = pack_infos.contiguous()        # itself when it is contiguous: the mark_ordered tag stays
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (sdf, inv_s, appends)):
        return _SdfToAlpha.apply(sdf, inv_s, appends, (pack_infos, bool(append_cdf_1)))
    detach = lambda t: t.detach() if isinstance(t, torch.Tensor) else t     # noqa: E731
    return _backend.sdf_to_alpha_forward(sdf.detach(), detach(inv_s), pack_infos, bool(append_cdf_1), detach(appends))


def neus_ray_sdf_to_alpha(sdf: torch.Tensor, inv_s, append_cdf_1=False, fused: bool = None):
    """``fused``: None follows FUSED_SDF_TO_ALPHA, False always takes the chain"""
    alpha = _fused_sdf_to_alpha(fused, sdf, inv_s, None, append_cdf_1, None)
    if alpha is not None:
        return alpha
    return neus_ray_cdf_to_alpha(neus_cdf(sdf, inv_s), append_cdf_1=append_cdf_1)


def neus_ray_sdf_to_tau(sdf: torch.Tensor, inv_s, append_cdf_1=False):
    """optical depth of every interval: drop of log sigmoid(sdf * inv_s), clamped at 0 (neus_utils.py:67-73)"""
    logcdf = F.logsigmoid(sdf * inv_s)
    append = sdf.new_zeros((*sdf.shape[:-1], 1)) if append_cdf_1 else None      # log(cdf = 1) = 0
    return (-torch.diff(logcdf, append=append)).clamp_min(0)


def neus_ray_sdf_to_vw(sdf: torch.Tensor, inv_s, append_cdf_1=False):
    return ray_alpha_to_vw(neus_ray_sdf_to_alpha(sdf, inv_s, append_cdf_1=append_cdf_1))


def neus_packed_cdf_to_alpha(cdf: torch.Tensor, pack_infos: torch.Tensor, append_cdf_1=False,
                             pack_cdf_appends: torch.Tensor = None):
    if append_cdf_1:
        pack_cdf_appends = cdf.new_ones(pack_infos.shape[0])
    drop = -packed_diff(cdf, pack_infos, pack_appends=pack_cdf_appends)
    return (drop / (cdf + 1e-5)).clamp_min(0)


def neus_packed_sdf_to_alpha(sdf: torch.Tensor, inv_s, pack_infos: torch.Tensor, append_cdf_1=False,
                             pack_sdf_appends: torch.Tensor = None, fused: bool = None):
    """``fused``: None follows FUSED_SDF_TO_ALPHA, False always takes the chain"""
    alpha = _fused_sdf_to_alpha(fused, sdf, inv_s, pack_infos, append_cdf_1, pack_sdf_appends)
    if alpha is not None:
        return alpha
    appends = None if pack_sdf_appends is None else neus_cdf(pack_sdf_appends, inv_s)
    return neus_packed_cdf_to_alpha(neus_cdf(sdf, inv_s), pack_infos, append_cdf_1=append_cdf_1, pack_cdf_appends=appends)


def neus_packed_sdf_to_tau(sdf: torch.Tensor, inv_s, pack_infos: torch.Tensor, append_cdf_1=False,
                           pack_sdf_appends: torch.Tensor = None):
    logcdf = F.logsigmoid(sdf * inv_s)
    if append_cdf_1:
        appends = sdf.new_zeros(pack_infos.shape[0])
    else:
        appends = None if pack_sdf_appends is None else F.logsigmoid(pack_sdf_appends * inv_s)
    return (-packed_diff(logcdf, pack_infos, pack_appends=appends)).clamp_min(0)


def neus_packed_sdf_to_vw(sdf: torch.Tensor, inv_s, pack_infos: torch.Tensor, append_cdf_1=False,
                          pack_sdf_appends: torch.Tensor = None):
    return packed_alpha_to_vw(neus_packed_sdf_to_alpha(sdf, inv_s, pack_infos, append_cdf_1=append_cdf_1,
                                                       pack_sdf_appends=pack_sdf_appends), pack_infos)


def neus_estimate_sdf_nablas_to_alpha(sdf: torch.Tensor, deltas: torch.Tensor, nablas: torch.Tensor, dirs: torch.Tensor,
                                      inv_s: Union[float, torch.Tensor], dir_scales: torch.Tensor = 1, ratio: float = 1,
                                      delta_max: float = 1e+10) -> torch.Tensor:
    """the original NeuS opacity: sdf [...] at the interval's sample moved half an interval (``deltas * dir_scales``, at most
    ``delta_max``) back and forth along the slope ``dirs . nablas`` (dirs normalised; only its negative part counts, annealed by
    ``ratio``) -> alpha [...] (neus_utils.py:121-158)"""
    true_cos = (dirs * nablas).sum(-1, keepdim=True)
    if ratio == 1:
        iter_cos = -F.relu(-true_cos)
    elif ratio == 0:
        iter_cos = -F.relu(-true_cos * 0.5 + 0.5)
    else:
        iter_cos = -(F.relu(-true_cos * 0.5 + 0.5) * (1.0 - ratio) + F.relu(-true_cos) * ratio)
    half = deltas.new_tensor([-0.5, 0.5]) * (deltas * dir_scales).unsqueeze(-1).clamp_max(delta_max)
    cdf = torch.sigmoid(torch.addcmul(sdf.unsqueeze(-1), iter_cos, half) * inv_s)
    return ((cdf[..., 0] - cdf[..., 1]) / (cdf[..., 0] + 1e-5)).clamp_min(0)


@torch.no_grad()
def neus_packed_sdf_to_upsample_alpha(sdf: torch.Tensor, depth_samples: torch.Tensor, inv_s, pack_infos: torch.Tensor):
    """the NeuS paper's up-sampling opacity: sdf at both interval ends re-estimated from the mid-point value and the
    smaller (more negative) of the current / previous slopes, clamped to [-10, 0] (neus_utils.py:164-189)"""
    d_sdf = packed_diff(sdf, pack_infos)                      # trailing zero in every pack
    deltas = packed_diff(depth_samples, pack_infos)
    slope = d_sdf / (deltas + 1e-5)
    prev = slope.roll(1).index_fill_(0, pack_infos[:, 0], 0)  # previous interval's slope, 0 at pack starts
    slope = torch.minimum(prev, slope).clamp_(-10, 0)
    mid = (sdf + d_sdf * 0.5).to(depth_samples.dtype)
    half = slope * deltas * 0.5
    cdf_prev, cdf_next = torch.sigmoid((mid - half) * inv_s), torch.sigmoid((mid + half) * inv_s)
    return ((cdf_prev - cdf_next) / (cdf_prev + 1e-5)).clamp_min_(0)


@torch.no_grad()
def neus_ray_sdf_to_upsample_alpha(sdf: torch.Tensor, depth_samples: torch.Tensor, inv_s) -> torch.Tensor:
    """batched form of the above: sdf, depth_samples [..., n] at the interval boundaries -> alpha [..., n-1] (neus_utils.py:190-217)"""
    deltas = depth_samples.diff(dim=-1)
    mid = (sdf[..., :-1] + sdf[..., 1:]) * 0.5
    slope = sdf.diff(dim=-1) / (deltas + 1e-5)
    prev = torch.cat([slope.new_zeros((*slope.shape[:-1], 1)), slope[..., :-1]], -1)
    slope = torch.minimum(prev, slope).clamp_(-10.0, 0.0)
    cdf = torch.sigmoid(torch.addcmul(mid.unsqueeze(-1), slope.unsqueeze(-1), deltas.unsqueeze(-1) * deltas.new_tensor([-0.5, 0.5])) * inv_s)
    return ((cdf[..., 0] - cdf[..., 1]) / (cdf[..., 0] + 1e-5)).clamp_min_(0)
