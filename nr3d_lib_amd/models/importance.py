"""nr3d_lib_amd.models.importance -- pixel importance sampling by 2D inverse-CDF sampling on accumulated error maps: ``ErrorMap`` and
``ImpSampler`` with the constructor signatures, attributes, buffers and methods of nr3d_lib/models/importance.py, whose checkpoints
load with ``strict=True``.

Conventions (the reference's): x, y are floats in [0, 1]; w, h are integers in [0, W-1], [0, H-1]; x <=> w, y <=> h.

Two routes, chosen per call:

* the CHAIN -- the reference's torch statements in the reference's order, down to the order and shapes of its ``torch.rand`` /
  ``torch.randint`` calls, so that a seeded CPU run returns the reference's own numbers.  CPU tensors, maps that are not float32,
  ``FUSED_IMPORTANCE = False`` and the calls not named in ``FUSED_CALLS`` take it;
* the FUSED route -- the kernels of csrc/importance.hip (bindings/_importance.py): one launch per sampling call (for ``ImpSampler`` one
  launch for the uniform share and all maps), an ACCUMULATING and reproducible update in two launches, the CDFs in three.  It draws
  the uniforms of a sampling call with one ``torch.rand([3, num_samples])`` (rows: image, x, y), so with one seed the two routes draw
  different samples of the same distribution.

Everything deterministic is in the functional helpers ``errmap_sample_from_uniform``, ``errmap_update`` and ``errmap_construct_cdf``,
which take the uniforms as arguments and run either route (``fused=``); the tests compare the two through them.

Where the routes differ on purpose: the chain's ``error_map[i, h, w] += ...`` is a non-accumulating ``index_put_`` --
of two samples of one call in one cell one contribution survives, which one is unspecified; the fused update adds all of them, and
gives the same bytes run after run.  A sample with a frame outside [0, N), a non-finite x, y or val, or a negative val is dropped by
the fused update and raises or writes garbage in the chain."""
from numbers import Number
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from nr3d_lib_amd.bindings import _importance as B

__all__ = ["ErrorMap", "ImpSampler", "errmap_sample_from_uniform", "errmap_update", "errmap_construct_cdf", "errmap_min_cdfs",
           "imp_segments"]

# the fused route, for float32 maps on the GPU; False: the chain everywhere.  FUSED_CALLS: the calls that take it when it is on
# (a call is listed when its slowest fused round beat the chain's fastest one in every row tools/exp_importance.py measures).
# profiles/importance.json: all three calls win in all 20 rows (4.1x to 11.9x), so all three are on.
FUSED_IMPORTANCE = True
FUSED_CALLS = frozenset({"sample", "update", "construct_cdf"})
# the reference's `assert not (val < 0).any()` in update_error_map -- a host wait; True is the reference's behaviour, on both routes
CHECK_VAL = True
# the fused update's int64 scratch has the map's shape; a map whose scratch would be larger than this takes the chain
UPDATE_SCRATCH_MAX_BYTES = 2 ** 30

U_MIN, U_MAX = 1e-6, 1 - 1e-6


def _fusable(*tensors) -> bool:
    dev = tensors[0].device
    return all(t.is_cuda and t.dtype == torch.float32 and t.device == dev for t in tensors)


def _on(call: str) -> bool:
    return FUSED_IMPORTANCE and call in FUSED_CALLS


# ---- the functional helpers ------------------------------------------------------------------------------------------------------
def errmap_sample_from_uniform(cdf_img: Optional[torch.Tensor], cdf_y: torch.Tensor, cdf_x_cond_y: torch.Tensor,
                               frame_ind: Union[None, int, torch.Tensor], u_img: Optional[torch.Tensor], u_x: Optional[torch.Tensor],
                               u_y: Optional[torch.Tensor], fused: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The frames ``i`` and pixel positions ``xy`` [n, 2] that the uniforms select: ``i`` is ``frame_ind`` (an int, or int64 [n]) or,
    with ``frame_ind`` None, the lower bound of ``u_img`` in ``cdf_img``; then y from ``cdf_y[i]`` and x from ``cdf_x_cond_y[i, h]``.
    ``u_x`` / ``u_y`` None: frames only, xy is None.  ``fused``: one launch of nr3d_importance_sample instead of the chain."""
    if fused:
        n = (u_img if u_img is not None else u_x).shape[0]
        i, xy = B.sample([(cdf_img, cdf_y, cdf_x_cond_y)], [0], 0, cdf_y.shape[0], u_img, u_x, u_y, frame_ind, need_i=frame_ind is None,
                         need_xy=u_x is not None)
        return (frame_ind if frame_ind is not None else i), xy
    if frame_ind is None:
        frame_ind = torch.searchsorted(cdf_img, u_img, right=False)
    if u_x is None:
        return frame_ind, None
    res_y, res_x = cdf_x_cond_y.shape[-2:]
    h = torch.searchsorted(cdf_y[frame_ind], u_y.unsqueeze(-1), right=False).squeeze(-1)
    prev = torch.where(h > 0, cdf_y[frame_ind, h - 1], cdf_y.new_zeros([]))
    y = ((u_y - prev) / (cdf_y[frame_ind, h] - prev) + h) / res_y
    w = torch.searchsorted(cdf_x_cond_y[frame_ind, h], u_x.unsqueeze(-1), right=False).squeeze(-1)
    prev = torch.where(w > 0, cdf_x_cond_y[frame_ind, h, w - 1], cdf_x_cond_y.new_zeros([]))
    x = ((u_x - prev) / (cdf_x_cond_y[frame_ind, h, w] - prev) + w) / res_x
    return frame_ind, torch.stack([x, y], dim=-1)


def errmap_update(error_map: torch.Tensor, i: Union[int, torch.Tensor], xy: torch.Tensor, val: torch.Tensor,
                  acc: Optional[torch.Tensor] = None) -> None:
    """The bilinear update of ``error_map`` [N, H, W] in place.  ``acc`` None: the chain, four read-modify-write ``index_put_``s that
    do NOT accumulate within a call.  ``acc`` (int64, the map's shape, all zero): the fused update, which does, reproducibly."""
    if acc is not None:
        B.update(error_map, acc, i, xy.contiguous(), val.contiguous())
        return
    res_y, res_x = error_map.shape[-2:]
    x_img, y_img = xy.movedim(-1, 0)
    wf, hf = x_img * res_x, y_img * res_y
    w, h = wf.long(), hf.long()
    w_w, w_h = (wf - w), (hf - h)                     # before the clamp: x == 1 puts the whole value into column res_x - 2
    w.clamp_(0, res_x - 2)
    h.clamp_(0, res_y - 2)
    error_map[i, h, w] += (1 - w_h) * (1 - w_w) * val
    error_map[i, h + 1, w] += w_h * (1 - w_w) * val
    error_map[i, h, w + 1] += (1 - w_h) * w_w * val
    error_map[i, h + 1, w + 1] += w_h * w_w * val


def errmap_min_cdfs(n_images: int, res_y: int, res_x: int, dtype=torch.float, device=None):
    """the CDFs of the uniform pdf, which ``min_pdf`` mixes in: (min_cdf_x_cond_y [N, H, W], min_cdf_y [N, H], min_cdf_img [N])"""
    def ramp(n):
        return torch.arange(n, dtype=dtype, device=device).add_(1).div_(n)
    return ramp(res_x).tile(n_images, res_y, 1), ramp(res_y).tile(n_images, 1), ramp(n_images)


def errmap_construct_cdf(error_map: torch.Tensor, min_pdf: float, max_pdf: Optional[float] = None, min_cdfs=None, clean: bool = False,
                         fused: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(cdf_x_cond_y [N, H, W], cdf_y [N, H], cdf_img [N]) of ``error_map`` seen as a pdf; the map is clamped to ``max_pdf`` in place
    when that is given, and zeroed afterwards with ``clean``.  ``fused``: nr3d_importance_construct_cdf, whose summation order is
    fixed (torch's GPU cumsum documents none, so the two routes may differ in the last bits there)."""
    if fused:
        return B.construct_cdf(error_map, min_pdf, max_pdf, clean)
    if max_pdf is not None:
        error_map.clamp_max_(max_pdf)
    if min_cdfs is None:
        min_cdfs = errmap_min_cdfs(*error_map.shape, dtype=error_map.dtype, device=error_map.device)
    min_cdf_x_cond_y, min_cdf_y, min_cdf_img = min_cdfs
    cdf_x_cond_y = (error_map + 1e-10).cumsum(dim=2)
    cumu = pdf_y = cdf_x_cond_y[:, :, -1]
    cdf_x_cond_y = (1 - min_pdf) * cdf_x_cond_y / cumu.unsqueeze(-1) + min_pdf * min_cdf_x_cond_y
    cdf_y = pdf_y.cumsum(dim=1)
    cumu = pdf_img = cdf_y[:, -1]
    cdf_y = (1 - min_pdf) * cdf_y / cumu.unsqueeze(-1) + min_pdf * min_cdf_y
    cdf_img = pdf_img.cumsum(dim=0)
    cdf_img = (1 - min_pdf) * cdf_img / cdf_img[-1:] + min_pdf * min_cdf_img
    if clean:
        error_map.zero_()
    return cdf_x_cond_y, cdf_y, cdf_img


def imp_segments(num_samples: int, frac_uniform: float, fracs: List[float]) -> Tuple[int, List[int]]:
    """(n_uniform, [samples per map]): int(num * frac) per share, the last map takes the remainder"""
    n_uniform = int(num_samples * frac_uniform)
    n_error_map = [int(num_samples * frac) for frac in fracs]
    n_error_map[-1] = num_samples - (n_uniform + sum(n_error_map[:-1]))
    return n_uniform, n_error_map


def _uniforms(num_samples: int, device) -> torch.Tensor:
    """the fused route's one draw: float32 [3, n] (rows: image, x, y), clamped as the reference clamps its own"""
    return torch.rand([3, num_samples], dtype=torch.float32, device=device).clamp_(U_MIN, U_MAX)


class ErrorMap(nn.Module):
    def __init__(self, n_images: int, error_map_hw: Tuple[int, int], *, min_pdf: float = 0.01, max_pdf: float = None,
                 n_steps_init: int = 128, n_steps_max: int = None, n_steps_growth_factor: float = 1.5,
                 dtype=torch.float, device=None) -> None:
        """
        Args:
            n_images: number of images in the dataset.
            error_map_hw: resolution (H, W) of the error map, usually much coarser than the images.
            min_pdf: share of the uniform pdf mixed in, against all-zero or very small error maps.
            max_pdf: clamp of the accumulated errors from above; None: none.
            n_steps_init: the initial CDF update period (``n_steps_between_update``), in iterations.
            n_steps_max: the longest CDF update period; None: no limit.
            n_steps_growth_factor: the next period over the previous one.
        """
        super().__init__()
        self.dtype = dtype
        res_y, res_x = error_map_hw
        self.n_images, self.res_y, self.res_x = n_images, res_y, res_x
        self.register_buffer('error_map', torch.zeros([n_images, res_y, res_x], device=device, dtype=dtype), persistent=True)

        self.cdf_x_cond_y: torch.Tensor = None      # [N, H, W]
        self.cdf_y: torch.Tensor = None             # [N, H]
        self.cdf_img: torch.Tensor = None           # [N]

        self.min_pdf = min_pdf
        self.max_pdf = max_pdf
        min_cdf_x_cond_y, min_cdf_y, min_cdf_img = errmap_min_cdfs(n_images, res_y, res_x, dtype=dtype, device=device)
        self.register_buffer('min_cdf_x_cond_y', min_cdf_x_cond_y, persistent=False)
        self.register_buffer('min_cdf_y', min_cdf_y, persistent=False)
        self.register_buffer('min_cdf_img', min_cdf_img, persistent=False)

        self.n_steps_since_update = 0
        self.n_steps_growth_factor = n_steps_growth_factor
        self.n_steps_between_update = n_steps_init
        self.n_steps_max = n_steps_max

        self._update_acc: torch.Tensor = None       # the fused update's scratch: a plain attribute, not in the state dict

    @property
    def device(self) -> torch.device:
        return self.error_map.device

    # ---- route choices
    def _fused_sampling(self) -> bool:
        return (_on("sample") and self.cdf_img is not None
                and _fusable(self.error_map, self.cdf_img, self.cdf_y, self.cdf_x_cond_y))

    def _scratch(self) -> torch.Tensor:
        """the update's int64 scratch, all zero between calls; made on first use and again when the map has moved or changed shape"""
        acc, m = self._update_acc, self.error_map
        if acc is None or acc.device != m.device or acc.shape != m.shape:
            acc = self._update_acc = torch.zeros(m.shape, dtype=torch.int64, device=m.device)
        return acc

    def _fused_update(self, i, xy, val) -> bool:
        m = self.error_map
        if not (_on("update") and _fusable(m) and m.is_contiguous() and self.res_y >= 2 and self.res_x >= 2
                and m.numel() * 8 <= UPDATE_SCRATCH_MAX_BYTES):
            return False
        if not (_fusable(m, xy, val) and xy.shape[-1] == 2 and xy.shape[:-1] == val.shape):
            return False
        if isinstance(i, torch.Tensor):
            return i.dtype == torch.int64 and i.device == m.device and i.shape == val.shape and i.is_contiguous()
        return isinstance(i, Number)

    @torch.no_grad()
    def update_error_map(self, i: Union[int, torch.LongTensor], xy: torch.Tensor, val: torch.Tensor):
        """
        Args:
            i: frame indices, an int or int64 [...]
            xy: pixel coordinates in [0, 1], [..., 2]
            val: the non-negative error at each (i, xy), [...]
        """
        if CHECK_VAL:
            assert not (val < 0).any(), "Found negative err when updating error_map. Please make sure to pass only non-negative err."
        errmap_update(self.error_map, i, xy, val, acc=self._scratch() if self._fused_update(i, xy, val) else None)

    @torch.no_grad()
    def get_normalized_error_map(self, frame_ind=None):
        error_map = self.error_map[frame_ind] if frame_ind is not None else self.error_map
        if self.max_pdf is not None:
            error_map = error_map.clone().clamp_max_(self.max_pdf)
        else:
            error_map = error_map / error_map.max().clamp_min(1e-5)
        return error_map

    def _construct(self, clean: bool):
        fused = _on("construct_cdf") and _fusable(self.error_map) and self.error_map.is_contiguous() and self.error_map.numel() > 0
        self.cdf_x_cond_y, self.cdf_y, self.cdf_img = errmap_construct_cdf(
            self.error_map, self.min_pdf, self.max_pdf, (self.min_cdf_x_cond_y, self.min_cdf_y, self.min_cdf_img), clean=clean, fused=fused)

    @torch.no_grad()
    def construct_cdf(self):
        """the 2D CDFs of the current error maps seen as pdfs"""
        self._construct(clean=False)

    @torch.no_grad()
    def construct_cdf_and_clean_error_map(self):
        """the same, and the error maps start again from zero"""
        self._construct(clean=True)

    @torch.no_grad()
    def step_error_map(self, i: Union[int, torch.LongTensor], xy: torch.Tensor, val: torch.Tensor):
        self.update_error_map(i=i, xy=xy, val=val)
        self.n_steps_since_update += 1
        if self.n_steps_since_update >= self.n_steps_between_update:
            self.construct_cdf_and_clean_error_map()
            self.n_steps_since_update = 0
            self.n_steps_between_update = int(self.n_steps_growth_factor * self.n_steps_between_update)
            if self.n_steps_max is not None:
                self.n_steps_between_update = min(self.n_steps_between_update, self.n_steps_max)

    @torch.no_grad()
    def get_pdf_image(self) -> torch.Tensor:
        """[n_images] the pdf (pmf) of the image frames"""
        cdf_img = self.cdf_img
        return cdf_img.diff(prepend=cdf_img.new_zeros([1, ]))

    @torch.no_grad()
    def sample_pixel(self, num_samples: int, frame_ind: Union[int, torch.LongTensor]) -> torch.Tensor:
        """[num_samples, 2] pixel positions xy in [0, 1], drawn by 2D inverse-CDF sampling on the given frame(s): an int, or int64
        [num_samples]"""
        if self._fused_sampling() and (isinstance(frame_ind, Number) or (
                isinstance(frame_ind, torch.Tensor) and frame_ind.dtype == torch.int64 and frame_ind.device == self.device
                and frame_ind.shape == (num_samples,) and frame_ind.is_contiguous())):
            u = _uniforms(num_samples, self.device)
            return errmap_sample_from_uniform(None, self.cdf_y, self.cdf_x_cond_y, frame_ind, None, u[1], u[2], fused=True)[1]
        x, y = torch.rand([2, num_samples], dtype=self.dtype, device=self.device).clamp_(U_MIN, U_MAX)
        return errmap_sample_from_uniform(None, self.cdf_y, self.cdf_x_cond_y, frame_ind, None, x, y)[1]

    @torch.no_grad()
    def sample_img(self, num_samples: int) -> torch.Tensor:
        """[num_samples] frame indices, drawn by inverse-CDF sampling"""
        if self._fused_sampling():
            u = _uniforms(num_samples, self.device)
            return errmap_sample_from_uniform(self.cdf_img, self.cdf_y, self.cdf_x_cond_y, None, u[0], None, None, fused=True)[0]
        i = torch.rand([num_samples], device=self.device, dtype=self.dtype).clamp_(U_MIN, U_MAX)
        return errmap_sample_from_uniform(self.cdf_img, self.cdf_y, self.cdf_x_cond_y, None, i, None, None)[0]

    @torch.no_grad()
    def sample_img_pixel(self, num_samples: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """([num_samples], [num_samples, 2]) frame indices and pixel positions, drawn together"""
        if self._fused_sampling():
            u = _uniforms(num_samples, self.device)
            return errmap_sample_from_uniform(self.cdf_img, self.cdf_y, self.cdf_x_cond_y, None, u[0], u[1], u[2], fused=True)
        i = self.sample_img(num_samples)
        xy = self.sample_pixel(num_samples, i)
        return i, xy


class ImpSampler(nn.Module):
    def __init__(self, error_maps: Dict[str, Tuple[ErrorMap, float]] = {}, frac_uniform: float = 0.5) -> None:
        """``error_maps``: name -> (map, its share of the non-uniform samples); ``frac_uniform``: the share drawn uniformly"""
        super().__init__()
        error_map_names: List[str] = list(error_maps.keys())
        error_map_list: List[ErrorMap] = [v[0] for v in error_maps.values()]
        error_map_fracs: List[float] = [v[1] for v in error_maps.values()]
        for error_map in error_map_list:
            if error_map.cdf_img is None:
                error_map.construct_cdf()
        assert all(error_map_list[0].n_images == e.n_images for e in error_map_list), "`error_maps` should have the same `n_images`"
        self.error_maps: Dict[str, ErrorMap] = nn.ModuleDict(dict(zip(error_map_names, error_map_list)))
        self.n_images = error_map_list[0].n_images
        non_uniform_fracs = np.array(error_map_fracs)
        self.error_map_fracs = ((1 - frac_uniform) * non_uniform_fracs / non_uniform_fracs.sum()).tolist()
        self.frac_uniform = frac_uniform
        self.error_map_names = error_map_names

    @property
    def device(self) -> torch.device:
        return self.error_maps[self.error_map_names[0]].device

    @property
    def dtype(self):
        return self.error_maps[self.error_map_names[0]].dtype

    @torch.no_grad()
    def get_pdf_image(self) -> torch.Tensor:
        pdf_list = []
        if self.frac_uniform > 0:
            pdf_list.append(self.frac_uniform * torch.full((self.n_images,), 1. / self.n_images, dtype=self.dtype, device=self.device))
        for frac, error_map in zip(self.error_map_fracs, self.error_maps.values()):
            pdf_list.append(frac * error_map.get_pdf_image())
        return torch.stack(pdf_list, 0).sum(0)

    @torch.no_grad()
    def sample_img(self, num_samples: int) -> torch.Tensor:
        n_uniform, n_error_map = imp_segments(num_samples, self.frac_uniform, self.error_map_fracs)
        i = []
        if n_uniform > 0:
            i.append(torch.randint(self.n_images, [n_uniform, ], dtype=torch.long, device=self.device))
        for n, error_map in zip(n_error_map, self.error_maps.values()):
            if n > 0:
                i.append(error_map.sample_img(n))
        return torch.cat(i, dim=0)

    @torch.no_grad()
    def sample_pixel(self, num_samples: int, frame_ind: int) -> torch.Tensor:
        assert isinstance(frame_ind, Number), "`frame_ind` must be a single frame index"
        n_uniform, n_error_map = imp_segments(num_samples, self.frac_uniform, self.error_map_fracs)
        xy = []
        if n_uniform > 0:
            xy.append(torch.rand([n_uniform, 2], dtype=self.dtype, device=self.device).clamp_(U_MIN, U_MAX))
        for n, error_map in zip(n_error_map, self.error_maps.values()):
            if n > 0:
                xy.append(error_map.sample_pixel(n, frame_ind))
        return torch.cat(xy, dim=0)

    def _fused_sampling(self) -> bool:
        maps = list(self.error_maps.values())
        return (len(maps) <= B.MAX_MAPS and all(m._fused_sampling() for m in maps) and all(m.device == maps[0].device for m in maps))

    @torch.no_grad()
    def sample_img_pixel(self, num_samples: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """uniform share + error_map0 + error_map1 + ... = num_samples, in this order"""
        n_uniform, n_error_map = imp_segments(num_samples, self.frac_uniform, self.error_map_fracs)
        if num_samples > 0 and min(n_error_map) >= 0 and self._fused_sampling():
            return imp_sample_from_uniform(list(self.error_maps.values()), n_uniform, n_error_map, self.n_images,
                                           _uniforms(num_samples, self.device), fused=True)
        i, xy = [], []
        if n_uniform > 0:
            i.append(torch.randint(self.n_images, [n_uniform, ], dtype=torch.long, device=self.device))
            xy.append(torch.rand([n_uniform, 2], dtype=self.dtype, device=self.device).clamp_(U_MIN, U_MAX))
        for n, error_map in zip(n_error_map, self.error_maps.values()):
            if n > 0:
                _i, _xy = error_map.sample_img_pixel(n)
                i.append(_i)
                xy.append(_xy)
        return torch.cat(i, dim=0), torch.cat(xy, dim=0)


def imp_sample_from_uniform(maps: List[ErrorMap], n_uniform: int, n_error_map: List[int], n_images: int, u: torch.Tensor,
                            fused: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """What ``ImpSampler.sample_img_pixel`` returns for the uniforms ``u`` float32 [3, n] (rows: image, x, y): samples [0, n_uniform)
    are uniform -- i = min(int(u_img * n_images), n_images - 1), xy = (u_x, u_y) -- then one segment per map, in order.  ``fused``: ONE
    launch for all of it; otherwise the chain helper per segment and a ``cat``."""
    firsts = np.cumsum([n_uniform] + list(n_error_map[:-1])).tolist()
    if fused:
        return B.sample([(m.cdf_img, m.cdf_y, m.cdf_x_cond_y) for m in maps], firsts, n_uniform, n_images, u[0], u[1], u[2])
    i = [(u[0, :n_uniform] * n_images).long().clamp_max_(n_images - 1)]
    xy = [torch.stack([u[1, :n_uniform], u[2, :n_uniform]], dim=-1)]
    for m, b, n in zip(maps, firsts, n_error_map):
        if n <= 0:
            continue
        _i, _xy = errmap_sample_from_uniform(m.cdf_img, m.cdf_y, m.cdf_x_cond_y, None, u[0, b:b + n], u[1, b:b + n], u[2, b:b + n])
        i.append(_i)
        xy.append(_xy)
    return torch.cat(i, dim=0), torch.cat(xy, dim=0)
